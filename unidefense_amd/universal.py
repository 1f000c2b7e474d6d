"""A universal perturbation: ONE pattern delta of size eps for every image, fitted on a few batches and applied blindly:
UniversalRunner, universal_runner and the float64 restatements ref_uap_*.

Every other runner here (unidefense_amd/attack.py, spatial.py) makes a new perturbation for each image.  A deployed detector
also meets the threat that needs no per-image optimisation — an overlay, a camera-pipeline filter, a re-encode signature added
to every face (Moosavi-Dezfooli et al., "Universal adversarial perturbations"; Shafahi et al., "Universal adversarial
training") — and the question it poses is what one pattern costs on data it was not fitted on.

The rule, per iteration on a batch (x, y), with f_n the per-sample cross-entropy at clamp(x_n + delta, clip):
    w_n   = (f_n < beta) and (source is None or y_n == source)       the clamped-loss rule: who still steers the pattern
    gsum  = sum over the counted n of d f_n / d x_adv_n                in ascending n, fp32
    linf  : delta <- clamp(delta + step sign(gsum), -eps, eps)
    l2    : delta <- delta + step gsum / max(|gsum|_2, 1e-12), then scaled back onto |delta|_2 <= eps
    x_adv = clamp(x + delta, clip)
The clip's effect on d x_adv / d delta (zero where the clamp is active) is ignored, as in every PGD here: the gradient with
respect to x_adv is summed as it is.  The direction is invariant to the scale of gsum for both norms, so under data parallel a
plain sum of the ranks' gsum (the `reduce` hook) gives every rank the same delta.

What is new next to the per-sample runners: delta PERSISTS across calls and batches (reset() zeroes it), and the iteration
holds a reduction over the batch (csrc/universal.hip: ud_uap_control, ud_uap_reduce, ud_uap_update_linf, ud_uap_apply).  The
life cycle is _Runner's: call 1 runs eagerly, call 2 captures one iteration — forward + d/dx (_Runner._grad, fp32 or the frozen
half backward), control, reduce, update — later calls replay it `steps` times.
"""
import math

import torch

from .attack import (_arguments, _cached_runner, _refuse_clip, _refuse_count, _refuse_eps, _refuse_norm, _Runner,
                     cross_entropy_each, frozen)

SOURCES = (None, 0, 1)


def resolve_uap_step(eps, step=None):
    """step=None: eps / 10"""
    return float(eps) / 10.0 if step is None else float(step)


def _refuse_beta(beta):
    if beta is None or not float(beta) > 0.0:
        raise ValueError(f"beta must be > 0 (inf: every sample steers), got {beta!r}")


def _refuse_source(source):
    if source is not None and (isinstance(source, bool) or source not in (0, 1)):
        raise ValueError(f"source must be one of {SOURCES}, got {source!r}")


def _refuse_reduce(reduce):
    if reduce is not None and not callable(reduce):
        raise ValueError(f"reduce must be None or a callable (gsum) -> None that sums gsum in place over the ranks, got {reduce!r}")


# ---- float64 restatements of the four kernels' rules (tests compare the GPU with these) ------------------------------------------
def ref_uap_control(f, y, beta=math.inf, source=None):
    """w [N] bool: (f < beta) & (source is None or y == source); a NaN f is not counted"""
    w = f.double() < float(beta)
    return w if source is None else w & (y == int(source))


def ref_uap_reduce(g, w):
    """sum over the counted samples of g [N, ...] in float64: excluded samples are skipped, not multiplied by zero"""
    g = g.double()
    out = torch.zeros_like(g[0])
    for n in range(g.shape[0]):
        if bool(w[n]):
            out = out + g[n]
    return out


def ref_uap_update_linf(delta, gsum, step, eps):
    """clamp(delta + step sign(gsum), -eps, eps), sign(0) = 0, in float64"""
    return torch.clamp(delta.double() + float(step) * torch.sign(gsum.double()), -float(eps), float(eps))


def ref_uap_update_l2(delta, gsum, step, eps):
    """delta + step gsum / max(|gsum|_2, 1e-12), then scaled by min(1, eps / max(|.|_2, 1e-12)), in float64"""
    gsum = gsum.double()
    d = delta.double() + float(step) * gsum / max(float(gsum.norm()), 1e-12)
    return d * min(1.0, float(eps) / max(float(d.norm()), 1e-12))


def ref_uap_apply(delta, x, lo, hi):
    """clamp(x + delta, lo, hi) for every sample of x [N, ...], in float64"""
    return torch.clamp(x.double() + delta.double().reshape(1, *x.shape[1:]), float(lo), float(hi))


class UniversalRunner(_Runner):
    """runner = UniversalRunner(model, batch, size, norm="linf", eps=..., steps=1, ...); x_adv = runner(x, y).

    `steps` iterations of the module's rule on the batch (x, y), STARTING FROM THE delta THE RUNNER HOLDS (a fresh runner, or
    reset(): zeros); returns x_adv = clamp(x + delta, clip), a static buffer.  delta [3, size, size] fp32 persists across calls:
    a fit is a loop of calls over batches and epochs.  step=None: eps / 10.  beta: samples whose loss reached beta stop steering
    (inf: everyone does); source (None, 0 or 1): only samples of that label steer, e.g. source=1 is "make fakes pass".
    apply(x[, out]) adds delta to any [n, 3, size, size] batch on the device, no backward, n free.
    reduce=None: one hipGraph holds the iteration — _grad, ud_uap_control, ud_uap_reduce, the update (linf: ud_uap_update_linf,
    one launch; l2: ud_sample_sumsq, ud_attack_step_l2, ud_sample_sumsq, ud_uap_apply).  reduce=callable: two graphs with
    reduce(gsum) between them — the data-parallel hook: an all-reduce that sums gsum in place gives every rank the same delta.
    The clip's effect on d x_adv / d delta is ignored.

    history [steps, batch] (each iteration's f), counted [steps, batch] int32 (who steered) hold the LAST call's values; g (the
    last iteration's per-sample gradients), gsum, out: static buffers; args: the resolved arguments.  precision / grad_scale:
    as InputGradRunner."""
    _what = "UniversalRunner"

    def __init__(self, model, batch, size, norm="linf", eps=None, steps=1, step=None, beta=math.inf, source=None,
                 clip=(-1.0, 1.0), precision="fp32", grad_scale=None, reduce=None):
        _refuse_norm(norm)
        _refuse_eps(eps)
        _refuse_count("steps", steps, 1)
        _refuse_clip(clip)
        _refuse_beta(beta)
        _refuse_source(source)
        _refuse_reduce(reduce)
        self._init_model(model, batch, size, precision, lambda: self._init_loss("cross_entropy", grad_scale))
        self.objective = cross_entropy_each
        self.norm, self.eps, self.steps = norm, float(eps), int(steps)
        self.step = resolve_uap_step(eps, step)
        self.beta, self.source, self.reduce = float(beta), None if source is None else int(source), reduce
        self.lo, self.hi = float(clip[0]), float(clip[1])
        self.args = {"method": "universal", "norm": norm, "eps": self.eps, "steps": self.steps, "step": self.step,
                     "beta": self.beta, "source": self.source, "clip": (self.lo, self.hi), "precision": self.precision,
                     "grad_scale": self.grad_scale, "reduce": None if reduce is None else getattr(reduce, "__name__", repr(reduce))}
        self.delta = torch.zeros(3, self.size, self.size, dtype=torch.float32, device=self.device)
        self.update_graph = None
        self.x0 = self.x_adv = self.y = self.history = self.counted = self.gsum = None

    def reset(self):
        """delta back to zeros"""
        with torch.no_grad():
            self.delta.zero_()

    def _buffers(self, x, y):
        from . import kernels as K
        dev = self.device
        self.x0 = x.detach().clone().contiguous()
        self.x_adv = self.x0.clone().requires_grad_()             # the static leaf: clamp(x0 + delta)
        self.y = y.detach().clone()
        self.ist, self.w, self.history, self.counted = K.uap_state(self.batch, self.steps, dev)
        self.gsum = torch.zeros_like(self.delta)
        if self.norm == "l2":
            per = self.delta.numel()
            self._gss, self._dss = (torch.zeros(1, dtype=torch.float64, device=dev) for _ in range(2))
            self._ws = torch.zeros(max(K.sample_sumsq_ws_bytes(1, per) // 8, 1), dtype=torch.float64, device=dev)

    def _gradient(self):
        """forward + d/dx at x_adv, who steers, their gradients' sum: the iteration up to the reduce hook"""
        from . import kernels as K
        g, self.out, f = self._grad(self.x_adv, self._each)
        self.g = g = g.contiguous()
        K.uap_control(f.detach().float().contiguous(), self.y, self.w, self.ist, self.history, self.counted, self.beta, self.source)
        K.uap_reduce(g, self.w, self.gsum)

    def _update(self):
        """delta's step and projection and the new x_adv, from gsum"""
        from . import kernels as K
        if self.norm == "linf":
            K.uap_update_linf(self.delta, self.gsum, self.x0, self.x_adv, self.step, self.eps, self.lo, self.hi)
        else:
            d, gs = self.delta.view(1, -1), self.gsum.view(1, -1)
            K.sample_sumsq(gs, None, out=self._gss, ws=self._ws)
            K.attack_step_l2(d, gs, self._gss, self.step)
            K.sample_sumsq(d, None, out=self._dss, ws=self._ws)
            K.uap_apply(self.delta, self._dss, self.x0, self.x_adv, self.eps, self.lo, self.hi)

    def _iteration(self):
        """one iteration on the static buffers: what the single graph holds"""
        self._gradient()
        self._update()

    def _start(self, x, y):
        from . import kernels as K
        with torch.no_grad():
            self.x0.copy_(x)
            self.y.copy_(y)
            self.ist.zero_()                                      # every row of history and counted is written again
            K.uap_apply(self.delta, None, self.x0, self.x_adv, self.eps, self.lo, self.hi)

    def __call__(self, x, y):
        self._check(x, y)
        self.calls += 1
        with torch.enable_grad():
            if self.calls == 1:                                   # eager warm-up: the same launches, a valid fit
                self._buffers(x, y)
            elif self.graph is None:
                if self.reduce is None:
                    self.graph, = self._capture(self._iteration)
                else:
                    self.graph, self.update_graph = self._capture(self._gradient, self._update)
            self._start(x, y)
            if self.graph is None:
                with frozen(self.model):
                    for _ in range(self.steps):
                        self._gradient()
                        if self.reduce is not None:
                            self.reduce(self.gsum)
                        self._update()
                return self.x_adv.detach()
        for _ in range(self.steps):
            self.graph.replay()
            if self.reduce is not None:
                self.reduce(self.gsum)
                self.update_graph.replay()
        return self.x_adv.detach()

    @torch.no_grad()
    def apply(self, x, out=None):
        """clamp(x + delta, clip) for a cuda fp32 [n, 3, size, size] batch, any n: a new tensor, or `out` (like x; may be x)"""
        from . import kernels as K
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError(f"{self._what}.apply takes a cuda tensor")
        if x.dim() != 4 or x.shape[0] < 1 or tuple(x.shape[1:]) != self.shape[1:] or x.dtype != torch.float32:
            raise ValueError(f"input {tuple(x.shape)} {x.dtype} is no [n, {', '.join(map(str, self.shape[1:]))}] torch.float32 batch")
        if out is not None and (out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous()):
            raise ValueError("out must be a contiguous tensor like x")
        src = x.detach().contiguous()
        out = torch.empty_like(src) if out is None else out
        return K.uap_apply(self.delta, None, src, out, self.eps, self.lo, self.hi)


_universal_arguments = _arguments(UniversalRunner)


def universal_runner(model, *args, **kwargs):
    """The model's UniversalRunner for the full argument tuple (UniversalRunner's after the model), made on first use; at most
    _MAX_RUNNERS are kept, in a dictionary of their own.  The runner holds delta: the same arguments give the same pattern back.
    A callable `reduce` is keyed by identity (the runner keeps it alive, so the identity stays its own)."""
    a = _universal_arguments(*args, **kwargs)
    key = dict(a, reduce=None if a["reduce"] is None else id(a["reduce"]))
    return _cached_runner(model, "_ud_universal_runners", key, lambda: UniversalRunner(model, *a.values()))
