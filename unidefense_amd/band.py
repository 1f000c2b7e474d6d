"""In which frequency band is the model fragile: a per-plane 2-D DCT in HIP, band masks, and a band-limited L2 PGD runner —
dct_matrix, band_mask, dct2, idct2, band_project, band_filter, BandRunner, band_runner and the float64 restatements ref_*.

Every block of the model mixes a spatial branch with a spectral one, and forgery detectors lean on high-frequency traces that
a resize, a re-encode or a blur removes.  The other runners bound a perturbation's size; this one also bounds WHERE in the
spectrum it lives, so that the same budget eps can be spent band by band and the damage compared.

Definitions (S the image side, every [S, S] plane of a tensor on its own):
    D[u, i]    = c_u cos(pi (2 i + 1) u / (2 S)), c_0 = sqrt(1 / S), c_u = sqrt(2 / S): the orthonormal DCT-II matrix, made on
                 the host in float64 and handed to the device rounded once to fp32
    dct2(x)    = D X D^T                         idct2(Y) = D^T Y D
    band_mask  : [S, S] zeros and ones, one where lo <= r(u, v) < hi; r = sqrt(u^2 + v^2) / S ("radial") or max(u, v) / S
                 ("square"); hi None: no upper end.  DC is in the band exactly when lo == 0; adjacent bands partition the plane.
    band_project(x, mask) = idct2(mask (.) dct2(x))        band_filter(x, mask, clip) = its clamp

The attack is L2 only.  Its state is the perturbation's DCT coefficients w [N, 3, S, S] fp32, from zero.  D is orthonormal, so
|delta|_2 = |w|_2 and the ball is projected in the coefficient domain.  One iteration, per sample:
    g  = d f / d x_adv                               (_Runner._grad, fp32 or the frozen half backward)
    G  = mask (.) dct2(g)
    a  = step / max(|G|_2, 1e-12)                     (targeted: -step)
    n2 = |w|^2 + 2 a <w, G> + a^2 |G|^2              (three dots, double, fixed order)
    s  = min(1, eps / max(sqrt(max(n2, 0)), 1e-12))
    w  = s (w + a G)
    x_adv = clamp(x + idct2(w), clip)
The clip's effect on the gradient is ignored, as in every PGD here.  The stepped point's norm follows from three dots of the
OLD state, so the step and the projection are one pass over w (csrc/band.hip: ud_band_dots, ud_band_update), and x_adv comes
out of the inverse transform's epilogue (ud_plane_dct2 with base and clip).
"""
import math

import torch

from .attack import (_arguments, _cached_runner, _key, _objective_name, _refuse_clip, _refuse_count, _refuse_eps, _Runner,
                     cross_entropy_each, frozen, resolve_step)

NORMS = ("l2",)
SHAPES = ("radial", "square")
DEFAULT_BANDS = ((0.0, 1.0 / 8.0), (1.0 / 8.0, 1.0 / 4.0), (1.0 / 4.0, 1.0 / 2.0), (1.0 / 2.0, None))
MAX_SIZE = 480                       # ud_plane_dct2 keeps a [ceil32(S)][33] fp32 strip of the intermediate in LDS: 63360 bytes at 480


# ---- host side: the matrix and the masks -------------------------------------------------------------------------------------------
def dct_matrix(size):
    """D [size, size] float64 on the CPU"""
    _refuse_count("size", size, 2)
    S = int(size)
    i = torch.arange(S, dtype=torch.float64)
    D = torch.cos(math.pi * (2.0 * i.reshape(1, S) + 1.0) * i.reshape(S, 1) / (2.0 * S)) * math.sqrt(2.0 / S)
    D[0] = math.sqrt(1.0 / S)
    return D


def _refuse_band(lo, hi, shape):
    if shape not in SHAPES:
        raise ValueError(f"shape must be one of {SHAPES}, got {shape!r}")
    if lo is None or not (math.isfinite(float(lo)) and float(lo) >= 0.0):
        raise ValueError(f"band lo must be a finite number >= 0, got {lo!r}")
    if hi is not None and not float(lo) < float(hi):
        raise ValueError(f"band must be (lo, hi) with lo < hi (hi None: no upper end), got {(lo, hi)!r}")


def band_mask(size, lo, hi=None, shape="radial"):
    """[size, size] fp32 zeros and ones on the CPU: one where lo <= r(u, v) < hi"""
    _refuse_count("size", size, 2)
    _refuse_band(lo, hi, shape)
    S = int(size)
    u = torch.arange(S, dtype=torch.float64)
    r = (torch.sqrt(u.reshape(S, 1) ** 2 + u.reshape(1, S) ** 2) if shape == "radial"
         else torch.maximum(u.reshape(S, 1), u.reshape(1, S)).expand(S, S)) / S
    m = r >= float(lo)
    if hi is not None:
        m = m & (r < float(hi))
    return m.to(torch.float32)


_MATRICES = {}                       # (device, size) -> (D, D^T) fp32 on the device: the _MAX_MATRICES most recently used
_MAX_MATRICES = 8                    # the model has four sides; a runner keeps its own pair alive whatever is dropped here


def _matrices(device, size):
    key = (str(device), int(size))
    pair = _MATRICES.pop(key, None)
    if pair is None:
        D = dct_matrix(size)
        pair = (D.to(torch.float32).to(device).contiguous(), D.t().contiguous().to(torch.float32).to(device))
        while len(_MATRICES) >= _MAX_MATRICES:
            del _MATRICES[next(iter(_MATRICES))]
    _MATRICES[key] = pair                # most recently used last
    return pair


# ---- the public transforms: cuda fp32 [..., S, S] ----------------------------------------------------------------------------------
def _planes(x, what):
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32:
        raise ValueError(f"{what} takes a cuda fp32 tensor")
    if x.dim() < 2 or x.shape[-1] != x.shape[-2] or not 2 <= x.shape[-1] <= MAX_SIZE or x.numel() == 0:
        raise ValueError(f"{what} takes [..., S, S] planes with 2 <= S <= {MAX_SIZE}, got {tuple(x.shape)}")
    return x.detach().contiguous()


def _mask_for(mask, x, what):
    if mask is None:
        return None
    S = x.shape[-1]
    if not isinstance(mask, torch.Tensor) or tuple(mask.shape) != (S, S):
        raise ValueError(f"{what}: the mask must be a [{S}, {S}] tensor, got "
                         f"{tuple(mask.shape) if isinstance(mask, torch.Tensor) else type(mask).__name__}")
    return mask.detach().to(device=x.device, dtype=torch.float32).contiguous()


def dct2(x, mask=None, out=None):
    """mask (.) (D X D^T) for every [S, S] plane of x"""
    from . import kernels as K
    x = _planes(x, "dct2")
    return K.plane_dct2(x, *_matrices(x.device, x.shape[-1]), _mask_for(mask, x, "dct2"), out=out)


def idct2(y, mask=None, out=None):
    """D^T (mask (.) Y) D for every [S, S] plane of y"""
    from . import kernels as K
    y = _planes(y, "idct2")
    return K.plane_dct2(y, *_matrices(y.device, y.shape[-1]), _mask_for(mask, y, "idct2"), inverse=True, out=out)


def band_project(x, mask):
    """idct2(mask (.) dct2(x)): the part of x inside the band"""
    return idct2(dct2(x, mask))


def band_filter(x, mask, clip=(-1.0, 1.0)):
    """clamp(band_project(x, mask), clip): the image with everything outside the band removed"""
    _refuse_clip(clip)
    return band_project(x, mask).clamp_(float(clip[0]), float(clip[1]))


# ---- float64 restatements (tests compare the GPU with these) -----------------------------------------------------------------------
def ref_dct2(x, mask=None, inverse=False):
    """dct2 / idct2 of [..., S, S] in float64 on x's device, by the definition"""
    x = x.double()
    D = dct_matrix(x.shape[-1]).to(x.device)
    if inverse:
        return D.t() @ (x if mask is None else x * mask.double()) @ D
    y = D @ x @ D.t()
    return y if mask is None else y * mask.double()


def ref_band_dots(w, G):
    """[N, 3] float64: |w|^2, <w, G>, |G|^2 per sample"""
    w, G = w.double().flatten(1), G.double().flatten(1)
    return torch.stack([(w * w).sum(1), (w * G).sum(1), (G * G).sum(1)], 1)


def ref_band_update(w, G, step, eps, dots=None):
    """s (w + a G) per sample in float64, a and s from the three dots (dots [N, 3]: another source's, e.g. the GPU's own)"""
    dots = ref_band_dots(w, G) if dots is None else dots.double()
    shape = (-1,) + (1,) * (w.dim() - 1)
    ww, wg, gg = dots[:, 0], dots[:, 1], dots[:, 2]
    a = float(step) / torch.sqrt(gg).clamp_min(1e-12)
    n2 = ww + 2.0 * a * wg + a * a * gg
    s = (float(eps) / torch.sqrt(n2.clamp_min(0.0)).clamp_min(1e-12)).clamp_max(1.0)
    return s.reshape(shape) * (w.double() + a.reshape(shape) * G.double())


def ref_band_attack(forward_and_grad, x, y, mask, eps, steps, step, targeted=False, clip=(-1.0, 1.0)):
    """The runner's rule in float64.  forward_and_grad(x_adv, y) -> (f [N], d sum(f) / d x_adv).  Returns a dict: x_adv, coeff (the
    best of the steps + 1 visited points, the zero perturbation first), best_loss, loss0, history [steps + 1, N], norms
    [steps + 1, N] (|w|_2 at every visited point), x_last, w_last."""
    x = x.double()
    lo, hi = float(clip[0]), float(clip[1])
    w = torch.zeros_like(x)
    xa = x.clamp(lo, hi)
    sign = -1.0 if targeted else 1.0
    history, norms, best = [], [], None
    for k in range(int(steps) + 1):
        f, g = forward_and_grad(xa, y)
        f = f.double()
        history.append(f)
        norms.append(w.flatten(1).norm(dim=1))
        if best is None:
            best = {"f": f.clone(), "x": xa.clone(), "w": w.clone()}
        else:
            better = sign * f > sign * best["f"]
            sel = better.reshape(-1, 1, 1, 1)
            best = {"f": torch.where(better, f, best["f"]), "x": torch.where(sel, xa, best["x"]), "w": torch.where(sel, w, best["w"])}
        if k == int(steps):
            break
        w = ref_band_update(w, ref_dct2(g, mask), sign * float(step), eps)
        xa = (x + ref_dct2(w, inverse=True)).clamp(lo, hi)
    return {"x_adv": best["x"], "coeff": best["w"], "best_loss": best["f"], "loss0": history[0], "history": torch.stack(history),
            "norms": torch.stack(norms), "x_last": xa, "w_last": w}


def ref_leak(x_adv, x, mask):
    """the share of |x_adv - x|^2 outside the band, float64 [N]; 0 where x_adv == x"""
    d = x_adv.double() - x.double()
    den = (d * d).flatten(1).sum(1)
    out = ref_dct2(d, 1.0 - mask.double().to(d.device))
    return torch.where(den > 0, (out * out).flatten(1).sum(1) / den.clamp_min(torch.finfo(torch.float64).tiny), torch.zeros_like(den))


# ---- the runner --------------------------------------------------------------------------------------------------------------------
def _refuse_band_norm(norm):
    if norm not in NORMS:
        raise ValueError(f"norm must be one of {NORMS}, got {norm!r}")


class BandRunner(_Runner):
    """runner = BandRunner(model, batch, size, band=(lo, hi), eps=..., steps=10, ...); x_adv = runner(x, y).

    `steps` iterations of the module's rule from the zero perturbation, ascending the per-sample objective f of the true labels
    (objective: cross_entropy_each, "cross_entropy" for the same, or a callable (out, y) -> [batch]; targeted=True: descending it
    towards the labels y), the perturbation confined to the band (band_mask(size, lo, hi, shape)) and to |delta|_2 <= eps before
    the clip.  mask=: an explicit [size, size] tensor of zeros and ones instead of a band.  Either way the runner OWNS its mask,
    a device buffer `mask` that the graphs read: the given tensor is copied into it, never aliased, and set_mask(m) refills it,
    so one runner (one pair of graphs) serves every band — the engine's stage does.  step=None: resolve_step(eps, steps).  The life cycle is _Runner's: call 1 runs eagerly, call 2
    captures two hipGraphs, later calls replay them.  Graph 1, replayed `steps` times: forward + d/dx at the iterate
    (_Runner._grad), the keep-best of the point just scored (K.apgd_keep), ud_plane_dct2 forward with the mask, ud_band_dots,
    ud_band_update, ud_plane_dct2 inverse with base x and the clip.  Graph 2, once: the forward alone at the last point, its
    keep-best, and the measurements.  Candidate 0 is the zero perturbation, so best_loss >= loss0 holds exactly (targeted: <=).

    Static results that the next call overwrites: x_adv (returned: the best point), delta (x_adv - x), coeff (the best point's
    w), best_loss [N], loss0 [N], history [steps + 1, N] (f at every point visited), norm [N] float64 (|coeff|_2), leak [N]
    float64 (the share of |x_adv - x|^2 that lies outside the band after the clip, 0 where x_adv == x), g (the last gradient),
    out (the last forward's output); args: the resolved arguments.  precision / grad_scale: as InputGradRunner."""
    _what = "BandRunner"

    def __init__(self, model, batch, size, band=None, shape="radial", mask=None, eps=None, steps=10, step=None, targeted=False,
                 clip=(-1.0, 1.0), objective=cross_entropy_each, precision="fp32", grad_scale=None, norm="l2"):
        _refuse_band_norm(norm)
        _refuse_eps(eps)
        _refuse_count("steps", steps, 1)
        _refuse_count("size", size, 2)
        if size > MAX_SIZE:
            raise ValueError(f"size must be <= {MAX_SIZE} (the transform's strip lives in LDS), got {size!r}")
        _refuse_clip(clip)
        if (band is None) == (mask is None):
            raise ValueError(f"exactly one of band=(lo, hi) and mask= must be given, got band={band!r} and "
                             f"mask={'None' if mask is None else 'a tensor'}")
        if band is not None:
            if not isinstance(band, (tuple, list)) or len(band) != 2:
                raise ValueError(f"band must be (lo, hi) with lo < hi (hi None: no upper end), got {band!r}")
            _refuse_band(band[0], band[1], shape)
        else:
            if shape not in SHAPES:
                raise ValueError(f"shape must be one of {SHAPES}, got {shape!r}")
            if not isinstance(mask, torch.Tensor) or tuple(mask.shape) != (int(size), int(size)):
                raise ValueError(f"mask must be a [{int(size)}, {int(size)}] tensor, got "
                                 f"{tuple(mask.shape) if isinstance(mask, torch.Tensor) else type(mask).__name__}")
        if step is not None and math.isnan(float(step)):
            raise ValueError(f"step must be a number, got {step!r}")
        if not callable(objective) and objective != "cross_entropy":
            raise ValueError(f"objective must be 'cross_entropy' or a callable (out, y) -> [batch], got {objective!r}")
        self._init_model(model, batch, size, precision, lambda: self._init_loss("cross_entropy", grad_scale))
        self.objective = objective if callable(objective) else cross_entropy_each
        self.eps, self.steps = float(eps), int(steps)
        self.step = resolve_step(eps, self.steps, step)
        self.targeted = bool(targeted)
        self.lo, self.hi = float(clip[0]), float(clip[1])
        self.band = None if band is None else (float(band[0]), None if band[1] is None else float(band[1]))
        self.args = {"method": "band", "norm": "l2", "band": self.band, "shape": shape, "eps": self.eps, "steps": self.steps,
                     "step": self.step, "targeted": self.targeted, "clip": (self.lo, self.hi),
                     "objective": _objective_name(objective), "precision": self.precision, "grad_scale": self.grad_scale}
        self.mask = torch.empty(self.size, self.size, dtype=torch.float32, device=self.device)        # the runner's own
        self.set_mask(band_mask(self.size, self.band[0], self.band[1], shape) if band is not None else mask)
        self.D, self.Dt = _matrices(self.device, self.size)
        self.closing_graph = None
        self.x0 = self.x_adv = self.y = self.coeff = self.delta = self.history = None

    def set_mask(self, mask):
        """copy a [size, size] tensor of zeros and ones (any device, any dtype) into the mask the graphs read: the next call
        attacks inside it"""
        if not isinstance(mask, torch.Tensor) or tuple(mask.shape) != (self.size, self.size):
            raise ValueError(f"mask must be a [{self.size}, {self.size}] tensor, got "
                             f"{tuple(mask.shape) if isinstance(mask, torch.Tensor) else type(mask).__name__}")
        with torch.no_grad():
            self.mask.copy_(mask.detach())
        return self

    def _buffers(self, x, y):
        from . import kernels as K
        n, dev, per = self.batch, self.device, 3 * self.size * self.size
        self.x0 = x.detach().clone().contiguous()
        self._x = self.x0.clone().requires_grad_()                # the static leaf: the iterate clamp(x0 + idct2(w))
        self._xd = self._x.detach()
        self.y = y.detach().clone()
        self.w, self.G, self.coeff, self.delta, self.x_adv = (torch.zeros_like(self.x0) for _ in range(5))
        self.comp = torch.zeros_like(self.mask)                   # 1 - mask, refreshed by the closing graph
        self.history = torch.zeros(self.steps + 1, n, dtype=torch.float32, device=dev)
        self.loss0 = self.history[0]
        self._f, self._best, self.best_loss = (torch.zeros(n, dtype=torch.float32, device=dev) for _ in range(3))
        self._keep = torch.zeros(n, dtype=torch.int32, device=dev)
        self._dots = torch.zeros(n, 3, dtype=torch.float64, device=dev)
        self._num, self._den, self._nn, self.norm, self.leak = (torch.zeros(n, dtype=torch.float64, device=dev) for _ in range(5))
        self._ws = torch.zeros(max(K.band_dots_ws_bytes(n, per) // 8, 1), dtype=torch.float64, device=dev)
        self._ssws = torch.zeros(max(K.sample_sumsq_ws_bytes(n, per) // 8, 1), dtype=torch.float64, device=dev)

    def _visit(self, f):
        """the point just scored: f into the history's staging row; where it beats the best so far it becomes the best"""
        from . import kernels as K
        f = f.detach().float()
        self._f.copy_(f)
        fa = -f if self.targeted else f
        better = fa > self._best
        self._keep.copy_(better)
        self._best.copy_(torch.where(better, fa, self._best))
        K.apgd_keep(self.x_adv, self._xd, self._keep)
        K.apgd_keep(self.coeff, self.w, self._keep)

    def _iteration(self):
        """one iteration on the static buffers: what graph 1 holds"""
        from . import kernels as K
        g, self.out, f = self._grad(self._x, self._each)
        self.g = g = g.contiguous()
        with torch.no_grad():
            self._visit(f)
            K.plane_dct2(g, self.D, self.Dt, self.mask, out=self.G)
            K.band_dots(self.w, self.G, out=self._dots, ws=self._ws)
            K.band_update(self.w, self.G, self._dots, -self.step if self.targeted else self.step, self.eps)
            K.plane_dct2(self.w, self.D, self.Dt, None, inverse=True, out=self._xd, base=self.x0, clip=(self.lo, self.hi))

    def _closing(self):
        """the closing evaluation: forward only at the last point, its keep-best, then the measurements: what graph 2 holds"""
        from . import kernels as K
        with torch.no_grad(), self._nodes():
            f = self._each(self.model(self._x))
        with torch.no_grad():
            self._visit(f)
            self.best_loss.copy_(-self._best if self.targeted else self._best)
            torch.sub(self.x_adv, self.x0, out=self.delta)
            self.comp.copy_(1.0 - self.mask)
            K.plane_dct2(self.delta, self.D, self.Dt, self.comp, out=self.G)          # G is free after the last iteration
            K.sample_sumsq(self.G, None, out=self._num, ws=self._ssws)
            K.sample_sumsq(self.delta, None, out=self._den, ws=self._ssws)
            self.leak.copy_(torch.where(self._den > 0, self._num / self._den.clamp_min(torch.finfo(torch.float64).tiny),
                                        torch.zeros_like(self._den)))
            K.sample_sumsq(self.coeff, None, out=self._nn, ws=self._ssws)
            self.norm.copy_(torch.sqrt(self._nn))

    def _start(self, x, y):
        with torch.no_grad():
            self.x0.copy_(x)
            self.y.copy_(y)
            self.w.zero_()
            self.coeff.zero_()
            self._xd.copy_(x.clamp(self.lo, self.hi))             # the zero perturbation: clamp(x + idct2(0), clip)
            self.x_adv.copy_(self._xd)
            self._best.fill_(-math.inf)

    def __call__(self, x, y):
        self._check(x, y)
        self.calls += 1
        with torch.enable_grad():
            if self.calls == 1:                                   # eager warm-up: the same launches, a valid attack
                self._buffers(x, y)
            elif self.graph is None:
                self.graph, self.closing_graph = self._capture(self._iteration, self._closing)
            self._start(x, y)
            if self.graph is None:
                with frozen(self.model):
                    for k in range(self.steps):
                        self._iteration()
                        self.history[k].copy_(self._f)
                    self._closing()
            else:
                for k in range(self.steps):
                    self.graph.replay()
                    self.history[k].copy_(self._f)                # a device copy behind the replay: no synchronisation
                self.closing_graph.replay()
            self.history[self.steps].copy_(self._f)
        return self.x_adv


_band_arguments = _arguments(BandRunner)


def _band_keyed(a):
    """the bound arguments in their hashable form: the band as a tuple; an explicit mask only as the fact that there is one — a
    mask is contents, which the runner copies, and neither a tensor's address nor its values make a key"""
    return dict(a, band=tuple(a["band"]) if isinstance(a["band"], (list, tuple)) else a["band"], mask=a["mask"] is not None)


def band_key(*args, **kwargs):
    """arguments: BandRunner's after the model"""
    return _key(_band_keyed(_band_arguments(*args, **kwargs)))


def band_runner(model, *args, **kwargs):
    """The model's BandRunner for the full argument tuple (BandRunner's after the model), made on first use; at most
    _MAX_RUNNERS are kept, in a dictionary of their own.  With an explicit `mask` the other arguments are the key: there is ONE
    such runner per argument tuple, and every fetch copies the given mask into it (set_mask), so it attacks inside the mask of
    the latest fetch."""
    a = _band_arguments(*args, **kwargs)
    made = []
    r = _cached_runner(model, "_ud_band_runners", _band_keyed(a), lambda: made.append(1) or BandRunner(model, *a.values()))
    if a["mask"] is not None and not made:
        r.set_mask(a["mask"])
    return r
