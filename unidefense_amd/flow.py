"""A flow-field attack (stAdv) on a differentiable warp: flow_warp(), FlowRunner, flow_runner and the float64 restatements
ref_flow_*.

The pixel-value attacks (unidefense_amd/attack.py, universal.py) change what a pixel holds; SpatialRunner (spatial.py) moves
pixels, but only through a black-box search over a few hundred global affine maps.  Here every output pixel has a displacement
of its own, w [N, 2, S, S] in pixels (channel 0 the column, channel 1 the row displacement), the image is resampled bilinearly at
p + w(p), and w ascends the loss by its gradient (Xiao et al. 2018, "Spatially Transformed Adversarial Examples"): the field is
small and smooth, outside every L-p ball of pixel values, and has 2 S^2 degrees of freedom where the affine grid has 5.

The rule, per iteration, with f_n the per-sample objective at x_adv = warp(x, w) and g = d sum(f) / d x_adv:
    gw = s (gx, gy) - tau t        (gx, gy) = <g, d warp / d w> at the pixel, t the gradient of the smoothness term
                                   L_flow(w) = sum over neighbour pairs of sqrt(|w(p) - w(q)|^2 + tv_eps); s = -1: targeted
    w  <- clamp(w + step sign(gw), -max_flow, max_flow)
and the flow with the best f over the steps + 1 points visited (the zero flow first) is the result.  The output pixel depends
on w at that pixel alone, so the adjoint is a gather (csrc/flow.hip: ud_flow_warp, ud_flow_grad, ud_flow_control,
ud_flow_update; the rules and the order of their fp32 operations are in include/unidefense_hip.h).  In place of the paper's
L-BFGS on a penalty this is the signed-gradient ascent of every other runner here, with an L-infinity bound on the flow.
"""
import math

import torch

from .attack import (_arguments, _cached_runner, _key, _objective_name, _refuse_count, _Runner, cross_entropy_each, frozen,
                     resolve_step)
from .corrupt import _check_images


# ---- float64 restatements of the four kernels' rules (tests compare the GPU with these) ------------------------------------------
def _axis(q, S):
    """(i0 int64, f float64, inside bool) of the source coordinate q (fp32, already rounded once): the header's cell rule"""
    q = q.double()
    nan = torch.isnan(q)
    p = torch.where(nan, torch.zeros_like(q), q).clamp(0.0, float(S - 1))
    c = torch.floor(p).clamp(max=float(S - 2))
    f = torch.where(nan, q, p - c)
    return c.long().clamp(0, S - 2), f, (q > 0.0) & (q < float(S - 1))


def _cells(w, S):
    """the cells of a flow [N, 2, S, S]: q = fp32(index) + w in fp32, ONE rounding, then float64"""
    w = w.detach().to(torch.float32)
    idx = torch.arange(S, dtype=torch.float32, device=w.device)
    return _axis(idx.view(1, 1, S) + w[:, 0], S), _axis(idx.view(1, S, 1) + w[:, 1], S)


def _taps(x, x0, y0):
    """u00, u01, u10, u11 [N, 3, S, S] float64"""
    N, C, S, _ = x.shape
    flat = x.double().reshape(N, C, S * S)

    def at(dy, dx):
        i = ((y0 + dy) * S + (x0 + dx)).reshape(N, 1, S * S).expand(N, C, S * S)
        return flat.gather(2, i).reshape(N, C, S, S)
    return at(0, 0), at(0, 1), at(1, 0), at(1, 1)


def ref_flow_warp(x, w):
    """x [N, 3, S, S] sampled bilinearly at p + w(p) (w [N, 2, S, S] in pixels; coordinates clamped to the image), in float64
    from the fp32 coordinate: (1 - fy) ((1 - fx) u00 + fx u01) + fy ((1 - fx) u10 + fx u11)"""
    S = x.shape[-1]
    (x0, fx, _), (y0, fy, _) = _cells(w, S)
    u00, u01, u10, u11 = _taps(x, x0, y0)
    fx, fy = fx.unsqueeze(1), fy.unsqueeze(1)
    return (1.0 - fy) * ((1.0 - fx) * u00 + fx * u01) + fy * ((1.0 - fx) * u10 + fx * u11)


def ref_flow_grad(g, x, w):
    """[N, 2, S, S] float64: d <g, warp(x, w)> / dw.  Zero where the coordinate is clamped (0 < q < S - 1 is strict)."""
    S = x.shape[-1]
    (x0, fx, inx), (y0, fy, iny) = _cells(w, S)
    u00, u01, u10, u11 = _taps(x, x0, y0)
    fx, fy, g = fx.unsqueeze(1), fy.unsqueeze(1), g.double()
    gx = (g * ((1.0 - fy) * (u01 - u00) + fy * (u11 - u10))).sum(1)
    gy = (g * ((1.0 - fx) * (u10 - u00) + fx * (u11 - u01))).sum(1)
    zero = torch.zeros_like(gx)
    return torch.stack([torch.where(inx, gx, zero), torch.where(iny, gy, zero)], 1)


def ref_flow_tv(w, tv_eps=1e-8):
    """(L_flow [N], its gradient [N, 2, S, S]) in float64: L_flow = sum over the unordered horizontal and vertical neighbour
    pairs of sqrt(|w(p) - w(q)|^2 + tv_eps); the gradient at p is the gather sum_q (w(p) - w(q)) / sqrt(|w(p) - w(q)|^2 + tv_eps)"""
    w = w.detach().double()
    t = torch.zeros_like(w)
    dh = w[:, :, :, 1:] - w[:, :, :, :-1]                            # right minus left
    dv = w[:, :, 1:, :] - w[:, :, :-1, :]                            # lower minus upper
    nh = torch.sqrt((dh * dh).sum(1, keepdim=True) + float(tv_eps))
    nv = torch.sqrt((dv * dv).sum(1, keepdim=True) + float(tv_eps))
    t[:, :, :, 1:] += dh / nh
    t[:, :, :, :-1] -= dh / nh
    t[:, :, 1:, :] += dv / nv
    t[:, :, :-1, :] -= dv / nv
    return nh.flatten(1).sum(1) + nv.flatten(1).sum(1), t


def ref_flow_control(f, k, best, maximise=True):
    """(keep [N] bool, best [N]) of one step of the keep-best rule at counter k: keep = k == 0, or f strictly better than best,
    or best NaN and f not"""
    f, best = f.double(), best.double()
    better = f > best if maximise else f < best
    keep = better | (torch.isnan(best) & ~torch.isnan(f)) | torch.full_like(better, k == 0)
    return keep, torch.where(keep, f, best)


def ref_flow_update(w, w_best, gw, keep, step, bound):
    """(w_new, w_best_new) in float64: w_best = w where keep[n]; w_new = clamp(w + step sign(gw), -bound, bound), sign(0) = 0,
    a NaN in gw becomes a NaN in w_new (torch.sign alone gives 0 for it)"""
    w, w_best, gw = w.double(), w_best.double(), gw.double()
    kept = keep.bool().view(-1, 1, 1, 1)
    sign = torch.where(torch.isnan(gw), gw, torch.sign(gw))
    return torch.clamp(w + float(step) * sign, -float(bound), float(bound)), torch.where(kept, w, w_best)


# ---- the warp as an operator ---------------------------------------------------------------------------------------------------
@torch.no_grad()
def flow_warp(x, w, out=None):
    """x resampled at p + w(p): a new tensor (or `out`, which must not be x) like x, a cuda fp32 [N, 3, S, S] batch with S >= 2;
    w: a cuda fp32 [N, 2, S, S] flow in pixels (channel 0 the column, channel 1 the row displacement).  Bilinear, coordinates
    clamped to the image (torch's grid_sample with padding_mode="border", align_corners=True at grid = 2 (p + w) / (S - 1) - 1).
    One launch; x is not changed."""
    _check_images(x, "flow_warp")
    if x.shape[2] < 2:
        raise ValueError(f"flow_warp takes images of size >= 2, got {tuple(x.shape)}")
    if not isinstance(w, torch.Tensor) or w.device != x.device or w.dtype != torch.float32 \
            or tuple(w.shape) != (x.shape[0], 2, x.shape[2], x.shape[3]):
        raise ValueError(f"the flow must be an fp32 [{x.shape[0]}, 2, {x.shape[2]}, {x.shape[3]}] tensor on x's device, got "
                         f"{tuple(w.shape) if isinstance(w, torch.Tensor) else type(w).__name__}")
    if out is not None and (out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous()
                            or out.data_ptr() == x.data_ptr()):
        raise ValueError("out must be a contiguous tensor like x and not x itself")
    from . import kernels as K
    src = x.detach().contiguous()
    out = torch.empty_like(src) if out is None else out
    return K.flow_warp(src, w.detach().contiguous(), out)


def _refuse_amount(name, v):
    if v is None or not (math.isfinite(float(v)) and float(v) >= 0.0):
        raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")


class FlowRunner(_Runner):
    """runner = FlowRunner(model, batch, size, max_flow=2.0, steps=20, ...); x_adv = runner(x, y).

    `steps` iterations of the module's rule from the zero flow, ascending the per-sample objective f of the true labels
    (objective="cross_entropy": each sample's loss; or a callable (out, y) -> [batch]; targeted=True: descending it towards the
    labels y).  max_flow: the L-infinity bound on every displacement component, in pixels; step=None: resolve_step(max_flow,
    steps); tau weighs the smoothness term, tv_eps smooths its root.  The life cycle is APGDRunner's: call 1 runs eagerly, call 2
    captures two hipGraphs, later calls replay them.  Graph 1, replayed `steps` times: forward + d/dx at x_adv (_Runner._grad,
    fp32 or the frozen half backward), ud_flow_grad, ud_flow_control, ud_flow_update — three launches behind the backward.
    Graph 2, once: the forward alone at the last x_adv, control, and the update's closing pass, which warps x by the best flow.
    Candidate 0 is the zero flow, so best_loss >= loss0 holds exactly (targeted: <=).

    Static results that the next call overwrites: x_adv (returned: the best flow's image), flow [N, 2, size, size] (the best
    flow), best_loss [N], loss0 [N] (f of the clean image), history [steps + 1, N] (f at every point visited), flow_linf [N]
    (max |flow|) and flow_tv [N] (L_flow of the best flow), g (the last gradient), out (the last forward's output); args: the
    resolved arguments.  precision / grad_scale: as InputGradRunner."""
    _what = "FlowRunner"

    def __init__(self, model, batch, size, max_flow=2.0, steps=20, step=None, tau=0.05, tv_eps=1e-8, targeted=False,
                 objective="cross_entropy", precision="fp32", grad_scale=None):
        _refuse_amount("max_flow", max_flow)
        _refuse_amount("tau", tau)
        if tv_eps is None or not (math.isfinite(float(tv_eps)) and float(tv_eps) > 0.0):
            raise ValueError(f"tv_eps must be a finite number > 0, got {tv_eps!r}")
        _refuse_count("steps", steps, 1)
        _refuse_count("size", size, 2)
        if step is not None and math.isnan(float(step)):
            raise ValueError(f"step must be a number, got {step!r}")
        if not callable(objective) and objective != "cross_entropy":
            raise ValueError(f"objective must be 'cross_entropy' or a callable (out, y) -> [batch], got {objective!r}")
        self._init_model(model, batch, size, precision, lambda: self._init_loss("cross_entropy", grad_scale))
        self.objective = objective if callable(objective) else cross_entropy_each
        self.max_flow, self.steps = float(max_flow), int(steps)
        self.step = resolve_step(max_flow, self.steps, step)
        self.tau, self.tv_eps, self.targeted = float(tau), float(tv_eps), bool(targeted)
        self.args = {"method": "flow", "max_flow": self.max_flow, "steps": self.steps, "step": self.step, "tau": self.tau,
                     "tv_eps": self.tv_eps, "targeted": self.targeted, "objective": _objective_name(objective),
                     "precision": self.precision, "grad_scale": self.grad_scale}
        self.closing_graph = None
        self.x0 = self.x_adv = self.y = self.flow = self.history = None

    def _buffers(self, x, y):
        from . import kernels as K
        n, dev = self.batch, self.device
        self.x0 = x.detach().clone().contiguous()
        self._x = self.x0.clone().requires_grad_()                # the static leaf: warp(x0, w)
        self.x_adv = self._x.detach()
        self.y = y.detach().clone()
        self.w = torch.zeros(n, 2, self.size, self.size, dtype=torch.float32, device=dev)
        self.flow, self.gw = torch.zeros_like(self.w), torch.zeros_like(self.w)
        self.ist, self.fst, self.history = K.flow_state(n, self.steps, dev)
        self._keep = self.ist[K.FLOW_I["keep"]]
        self.best_loss = self.fst[K.FLOW_F["f_best"]]
        self.loss0 = self.history[0]
        self.flow_linf = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flow_tv = torch.zeros(n, dtype=torch.float32, device=dev)

    def _control(self, f):
        from . import kernels as K
        K.flow_control(f.detach().float().contiguous(), self.ist, self.fst, self.history, maximise=not self.targeted)

    def _iteration(self):
        """one iteration on the static buffers: what graph 1 holds"""
        from . import kernels as K
        g, self.out, f = self._grad(self._x, self._each)
        self.g = g = g.contiguous()
        K.flow_grad(g, self.x0, self.w, self.gw, -1 if self.targeted else 1, self.tau, self.tv_eps)
        self._control(f)
        K.flow_update(self.w, self.flow, self.gw, self._keep, self.x0, self.x_adv, self.step, self.max_flow)

    def _closing(self):
        """the closing evaluation: forward only at the last point, then the best flow's image: what graph 2 holds"""
        from . import kernels as K
        with torch.no_grad(), self._nodes():
            f = self._each(self.model(self._x))
        self._control(f)
        K.flow_update(self.w, self.flow, None, self._keep, self.x0, self.x_adv, self.step, self.max_flow, closing=True)

    def __call__(self, x, y):
        self._check(x, y)
        self.calls += 1
        with torch.enable_grad():
            if self.calls == 1:                                   # eager warm-up: the same launches, a valid attack
                self._buffers(x, y)
            elif self.graph is None:
                self.graph, self.closing_graph = self._capture(self._iteration, self._closing)
            with torch.no_grad():
                self.x0.copy_(x)
                self.y.copy_(y)
                self.w.zero_()
                self.flow.zero_()
                self.ist.zero_()
                self.fst.zero_()
                self.history.zero_()
                self.x_adv.copy_(x)
            if self.graph is None:
                with frozen(self.model):
                    for _ in range(self.steps):
                        self._iteration()
                    self._closing()
            else:
                for _ in range(self.steps):
                    self.graph.replay()
                self.closing_graph.replay()
        with torch.no_grad():                                     # the best flow's size, by torch, after the replay
            self.flow_linf.copy_(self.flow.abs().flatten(1).amax(1))
            dh = self.flow[:, :, :, 1:] - self.flow[:, :, :, :-1]
            dv = self.flow[:, :, 1:, :] - self.flow[:, :, :-1, :]
            self.flow_tv.copy_(torch.sqrt((dh * dh).sum(1) + self.tv_eps).flatten(1).sum(1)
                               + torch.sqrt((dv * dv).sum(1) + self.tv_eps).flatten(1).sum(1))
        return self.x_adv


_flow_arguments = _arguments(FlowRunner)


def flow_key(*args, **kwargs):
    """arguments: FlowRunner's after the model"""
    return _key(_flow_arguments(*args, **kwargs))


def flow_runner(model, *args, **kwargs):
    """The model's FlowRunner for the full argument tuple (FlowRunner's after the model), made on first use; at most
    _MAX_RUNNERS are kept, in a dictionary of their own (the other runners' caches are untouched)."""
    a = _flow_arguments(*args, **kwargs)
    return _cached_runner(model, "_ud_flow_runners", a, lambda: FlowRunner(model, *a.values()))
