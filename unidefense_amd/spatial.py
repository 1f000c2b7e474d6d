"""Affine warps on the device and the worst-case spatial search: warp(), spatial_candidates() and SpatialRunner.

How robust is a detector to where the face sits in the frame?  Two face detectors, or one on two frames, cut crops that differ by
a few pixels of shift, a few degrees of roll, a few per cent of scale and sometimes a mirror.  The measurement is worst-of-grid
over rotations, translations and scales (Engstrom et al., "Exploring the landscape of spatial robustness"): it needs forwards
only.

The warp is defined like the corruptions (unidefense_amd/corrupt.py): on 8-bit grey levels, in exact integers, one launch
(csrc/warp.hip, include/unidefense_hip.h).  A transform is six int32 (affine_q16): the inverse of
p_out = scale R(angle) diag(flip ? -1 : 1, 1) p_src + shift in Q16, made here in float64; the kernel maps every output pixel's
centre to a source position in Q16 pixels, takes four taps through the border rule and blends them with 8-bit fractions.
tests/test_spatial_cpu.py restates it in numpy bit for bit.  The identity returns the quantised input, flip is the exact mirror,
an integer shift an exact shift, a right angle the exact rot90.

SpatialRunner follows SquareRunner's life cycle (unidefense_amd/attack.py): black-box, a per-sample state machine on the device,
one captured query — warp, eval forward, per-sample objective, control — replayed once per candidate.  No tape, no gradient,
nothing frozen, no early stop: the whole landscape `history` is the result, and the worst case is its minimum.
"""
import math

import torch

from .attack import (_Runner, _arguments, _cached_runner, _detached, _neg_cross_entropy_each, _objective_name, _refuse_count,
                     margin_each)
from .corrupt import _check_images, _hashable, _lut
from .infer import _check_precision, _eval_nodes

BORDERS = ("reflect", "edge", "fill")
SEARCHES = ("grid", "random")
SPATIAL_OBJECTIVES = ("margin", "cross_entropy")
_INT32 = 2 ** 31


# ---- host tables: float64 and integers only, the same on any machine ---------------------------------------------------------
def _q16(v):
    q = int(math.floor(v * 65536.0 + 0.5))
    if not -_INT32 <= q < _INT32:
        raise ValueError(f"the transform does not fit Q16 in int32: {v!r}")
    return q


def affine_q16(angle=0.0, scale=1.0, shift=(0.0, 0.0), flip=False):
    """(m00, m01, o0, m10, m11, o1): the six integers ud_warp_affine takes for the map
    p_out = A p_src + shift, A = scale R(angle) diag(flip ? -1 : 1, 1), R(a) = [[cos a, -sin a], [sin a, cos a]],
    x to the right, y down, angle in degrees, shift in pixels.  The kernel walks the output, so the integers are the INVERSE in
    float64: m = floor(A^-1 65536 + 0.5), o = floor(2 (-A^-1 shift) 65536 + 0.5) (the kernel's coordinates are half pixels)."""
    angle, scale, sx, sy = float(angle), float(scale), float(shift[0]), float(shift[1])
    if not all(math.isfinite(v) for v in (angle, scale, sx, sy)):
        raise ValueError(f"angle, scale and shift must be finite, got {angle!r}, {scale!r}, {(sx, sy)!r}")
    if not scale > 0.0:
        raise ValueError(f"scale must be > 0, got {scale!r}")
    c, s = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    f = -1.0 if flip else 1.0
    # A^-1 = diag(f, 1) R(-angle) / scale
    i00, i01, i10, i11 = f * c / scale, f * s / scale, -s / scale, c / scale
    return (_q16(i00), _q16(i01), _q16(2.0 * -(i00 * sx + i01 * sy)), _q16(i10), _q16(i11), _q16(2.0 * -(i10 * sx + i11 * sy)))


def _refuse_ranges(max_angle, max_shift, scales):
    if not (math.isfinite(float(max_angle)) and float(max_angle) >= 0.0):
        raise ValueError(f"max_angle must be a finite number >= 0 (degrees), got {max_angle!r}")
    if not (math.isfinite(float(max_shift)) and float(max_shift) >= 0.0):
        raise ValueError(f"max_shift must be a finite number >= 0 (a fraction of the side), got {max_shift!r}")
    if not isinstance(scales, (list, tuple)) or len(scales) != 2 or not 0.0 < float(scales[0]) <= float(scales[1]) < math.inf:
        raise ValueError(f"scales must be (lo, hi) with 0 < lo <= hi, got {scales!r}")


def _refuse_search(search, grid, k):
    if search not in SEARCHES:
        raise ValueError(f"search must be one of {SEARCHES}, got {search!r}")
    if search == "grid":
        if not isinstance(grid, (list, tuple)) or len(grid) != 3:
            raise ValueError(f"grid must be (angles, shifts, scales), three counts >= 1, got {grid!r}")
        for name, v in zip(("grid angles", "grid shifts", "grid scales"), grid):
            _refuse_count(name, v, 1)
    else:
        _refuse_count("k", k, 1)


def _linspace(lo, hi, count):
    """count >= 2 values from lo to hi in float64, both ends exact"""
    return [lo + (hi - lo) * i / (count - 1) if i < count - 1 else hi for i in range(count)]


def spatial_candidates(size, max_angle=10.0, max_shift=0.05, scales=(0.9, 1.1), flip=False, search="grid", grid=(7, 5, 3), k=64,
                       batch=1, generator=None):
    """The candidate table, float64 [K, batch, 5] of (angle in degrees, dx, dy in pixels, scale, flip 0 / 1).  Candidate 0 is the
    identity for every sample.
    search="grid", grid=(ga, gs, gz): K = 1 + ga gs gs gz (twice that product with flip); the same grid for every sample, in the
    order of nested loops flip (False, True) > angle > dx > dy > scale, the scale running fastest, over
    linspace(-max_angle, max_angle, ga), linspace(-max_shift size, max_shift size, gs) twice and linspace(scales[0], scales[1],
    gz).  A count of 1 means the neutral value: angle 0, shift 0, scale 1.
    search="random": K = 1 + k; k draws per sample, uniform on the same ranges, from a CPU generator (None: torch's default CPU
    generator) in this fixed order: u_angle, u_dx, u_dy, u_scale, each torch.rand [k, batch] float64, then, with flip only,
    torch.randint(0, 2) [k, batch]; value = lo + (hi - lo) u.  The same seed gives the same table on any machine."""
    _refuse_ranges(max_angle, max_shift, scales)
    _refuse_search(search, grid, k)
    _refuse_count("size", size, 1)
    _refuse_count("batch", batch, 1)
    size, batch = int(size), int(batch)
    a, t, lo, hi = float(max_angle), float(max_shift) * size, float(scales[0]), float(scales[1])
    identity = torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0], dtype=torch.float64)
    if search == "grid":
        ga, gs, gz = (int(v) for v in grid)
        angles = _linspace(-a, a, ga) if ga > 1 else [0.0]
        shifts = _linspace(-t, t, gs) if gs > 1 else [0.0]
        zooms = _linspace(lo, hi, gz) if gz > 1 else [1.0]
        rows = [[an, dx, dy, z, f] for f in ((0.0, 1.0) if flip else (0.0,)) for an in angles for dx in shifts for dy in shifts
                for z in zooms]
        table = torch.cat([identity.reshape(1, 5), torch.tensor(rows, dtype=torch.float64)], 0)
        return table.unsqueeze(1).repeat(1, batch, 1)
    if generator is not None and generator.device.type != "cpu":
        raise ValueError("a random search draws from a CPU generator: the same seed gives the same table on any machine")
    k = int(k)
    u = [torch.rand(k, batch, generator=generator, dtype=torch.float64) for _ in range(4)]
    f = torch.randint(0, 2, (k, batch), generator=generator).to(torch.float64) if flip else torch.zeros(k, batch, dtype=torch.float64)
    draws = torch.stack([-a + 2.0 * a * u[0], -t + 2.0 * t * u[1], -t + 2.0 * t * u[2], lo + (hi - lo) * u[3], f], 2)
    return torch.cat([identity.reshape(1, 1, 5).repeat(1, batch, 1), draws], 0)


def candidates_q16(cand):
    """int32 [K batch, 6]: affine_q16 of every row of a candidate table [K, batch, 5], candidate-major (row k batch + n)"""
    flat = cand.reshape(-1, 5).tolist()
    memo = {}
    rows = []
    for an, dx, dy, z, f in flat:
        key = (an, dx, dy, z, f)
        if key not in memo:
            memo[key] = affine_q16(an, z, (dx, dy), f != 0.0)
        rows.append(memo[key])
    return torch.tensor(rows, dtype=torch.int64).to(torch.int32)


def _per_sample(v, n, what, width=None):
    """v as a list of n python values (width: n tuples of that many): a scalar (one pair) serves every sample"""
    if hasattr(v, "tolist"):                                      # a tensor or an array
        v = v.tolist()
    one = not isinstance(v, (list, tuple)) if width is None else (len(v) == width and not isinstance(v[0], (list, tuple)))
    out = [v] * n if one else list(v)
    if len(out) != n or (width is not None and any(not isinstance(p, (list, tuple)) or len(p) != width for p in out)):
        raise ValueError(f"{what} takes one value or one per sample ({n}), got {v!r}")
    return out


def _refuse_border(border):
    if border not in BORDERS:
        raise ValueError(f"border must be one of {BORDERS}, got {border!r}")


@torch.no_grad()
def warp(x, angle=0.0, scale=1.0, shift=(0.0, 0.0), flip=False, border="reflect", out=None):
    """x warped by p_out = scale R(angle) diag(flip ? -1 : 1, 1) p_src + shift about the image's centre: a new tensor (or `out`,
    which must not be x) like x, a cuda fp32 [N, 3, S, S] batch in model units.  angle (degrees), scale, flip: a scalar or N
    values; shift (pixels, (dx, dy)): one pair or N pairs.  border: "reflect" (101), "edge" or "fill" (level 128).  One launch;
    x is not changed."""
    _refuse_border(border)
    _check_images(x, "warp")
    n = x.shape[0]
    table = [affine_q16(a, z, s, bool(f)) for a, z, s, f in zip(_per_sample(angle, n, "angle"), _per_sample(scale, n, "scale"),
                                                                  _per_sample(shift, n, "shift", 2), _per_sample(flip, n, "flip"))]
    if out is not None and (out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous()
                            or out.data_ptr() == x.data_ptr()):
        raise ValueError("out must be a contiguous tensor like x and not x itself")
    from . import kernels as K
    src = x.detach().contiguous()
    out = torch.empty_like(src) if out is None else out
    mat = torch.tensor(table, dtype=torch.int64).to(torch.int32).to(x.device)
    row = torch.arange(n, dtype=torch.int32, device=x.device)
    return K.warp_affine(src, out, _lut(x.device), mat, row, border)


class SpatialRunner(_Runner):
    """runner = SpatialRunner(model, batch, size, max_angle=10.0, ...); x_adv = runner(x, y[, generator]).

    The worst case over K spatial candidates (spatial_candidates: a grid, or k random draws per sample from the CPU `generator`;
    candidate 0 is the identity) of the per-sample objective f, which is MINIMISED (objective="margin": margin_each, the sample
    is fooled once f <= 0; "cross_entropy": minus each sample's loss; or a callable (out, y) -> [batch]).  One hipGraph holds ONE
    query — ud_warp_affine(x0 -> x_try) through the state's row, the eval forward (InferenceRunner's, either precision) under
    no_grad, f, ud_spatial_control — and a call replays it K times, then warps x0 once more by each sample's winner.  Call 1 runs
    eagerly, call 2 captures, later calls replay.  No early stop, no tape, no gradient, nothing frozen.

    Static results that the next call overwrites: x_adv (returned), best_loss [N] (the lowest f; ties keep the lowest k), best_k
    [N] int32, best [N, 5] (the winner's (angle, dx, dy, scale, flip): a float64 CPU tensor), loss0 [N] (the identity's f),
    history [K, N] (the landscape), out (the last forward's output); args: the resolved arguments; candidates: the last table."""
    _what = "SpatialRunner"
    _backward = False

    def __init__(self, model, batch, size, max_angle=10.0, max_shift=0.05, scales=(0.9, 1.1), flip=False, search="grid",
                 grid=(7, 5, 3), k=64, border="reflect", objective="margin", precision="fp32"):
        def arguments():
            _refuse_search(search, grid, k)
            _refuse_border(border)
            if not callable(objective) and objective not in SPATIAL_OBJECTIVES:
                raise ValueError(f"objective must be one of {SPATIAL_OBJECTIVES} or a callable (out, y) -> [batch], got {objective!r}")
            _refuse_ranges(max_angle, max_shift, scales)
        self._init_model(model, batch, size, precision, arguments)
        self.objective = objective if callable(objective) else (margin_each if objective == "margin" else _neg_cross_entropy_each)
        self.search, self.border, self.flip = search, border, bool(flip)
        self.max_angle, self.max_shift = float(max_angle), float(max_shift)
        self.scales = (float(scales[0]), float(scales[1]))
        self._search = (grid, k)                                             # as given: only the one `search` uses was checked
        self.grid, self.k = tuple(int(v) for v in grid) if search == "grid" else None, int(k) if search == "random" else None
        self._fixed = self._table(None) if search == "grid" else None       # a grid is the same table on every call
        self.K = self._fixed.shape[0] if search == "grid" else 1 + self.k
        self.args = {"method": "spatial", "max_angle": self.max_angle, "max_shift": self.max_shift, "scales": self.scales,
                     "flip": self.flip, "search": search, "grid": self.grid, "k": self.k, "candidates": self.K, "border": border,
                     "objective": _objective_name(objective), "precision": self.precision}
        self.x0 = self.x_try = self.x_adv = self.y = self.history = self.candidates = None

    def _table(self, generator):
        return spatial_candidates(self.size, self.max_angle, self.max_shift, self.scales, self.flip, self.search, *self._search,
                                  self.batch, generator)

    def _buffers(self, x, y):
        from . import kernels as K
        n, dev = self.batch, self.device
        self.x0 = x.detach().clone().contiguous()
        self.x_try, self.x_adv = torch.zeros_like(self.x0), torch.zeros_like(self.x0)
        self.y = y.detach().clone()
        self.ist, self.fst = K.spatial_state(n, dev)
        self.history = torch.zeros(self.K, n, dtype=torch.float32, device=dev)
        self.best_loss = torch.zeros(n, dtype=torch.float32, device=dev)
        self.loss0 = torch.zeros(n, dtype=torch.float32, device=dev)
        self.best_k = torch.zeros(n, dtype=torch.int32, device=dev)
        self.best = torch.zeros(n, 5, dtype=torch.float64)
        self._mat = torch.zeros(self.K * n, 6, dtype=torch.int32, device=dev)
        self._row = self.ist[K.SPATIAL_I["row"]]
        self._first = torch.arange(n, dtype=torch.int32, device=dev)
        self._lut = _lut(dev)

    def _warp(self, dst):
        from . import kernels as K
        K.warp_affine(self.x0, dst, self._lut, self._mat, self._row, self.border)

    def _iteration(self):
        """one query on the static buffers: what the graph holds"""
        from . import kernels as K
        self._warp(self.x_try)
        with torch.no_grad(), _eval_nodes(self.model, self.half):
            out = self.model(self.x_try)
            f = self._each(out)
        self.out = _detached(out)
        K.spatial_control(f.detach().float().contiguous(), self.ist, self.fst, self.history)

    def __call__(self, x, y, generator=None):
        from . import kernels as K
        self._check(x, y)
        cand = self._fixed if self._fixed is not None else self._table(generator)
        mat = candidates_q16(cand)
        self.calls += 1
        if self.calls == 1:                                       # eager warm-up: the same launches, a valid search
            self._buffers(x, y)
        elif self.graph is None:
            self.graph, = self._capture(self._iteration)
        with torch.no_grad():
            self.x0.copy_(x)
            self.y.copy_(y)
            self._mat.copy_(mat.to(self.device))
            self.ist.zero_()
            self.fst.zero_()
            self.history.zero_()
            self._row.copy_(self._first)
        for _ in range(self.K):
            if self.graph is None:
                self._iteration()
            else:
                self.graph.replay()
        # closing reads no f: any [N] fp32 buffer stands in for it
        K.spatial_control(self.best_loss, self.ist, self.fst, self.history, closing=True)
        self._warp(self.x_adv)
        with torch.no_grad():
            self.best_loss.copy_(self.fst[K.SPATIAL_F["f_best"]])
            self.best_k.copy_(self.ist[K.SPATIAL_I["best_k"]])
            self.loss0.copy_(self.history[0])
        self.candidates = cand
        self.best.copy_(cand[self.best_k.cpu().long(), torch.arange(self.batch)])
        return self.x_adv


_spatial_arguments = _arguments(SpatialRunner)


def spatial_runner(model, *args, **kwargs):
    """The model's SpatialRunner for the full argument tuple (SpatialRunner's after the model), made on first use; at most
    _MAX_RUNNERS are kept, in a dictionary of their own (the other runners' caches are untouched)."""
    a = _spatial_arguments(*args, **kwargs)
    _check_precision(model, a["precision"])
    key = dict(a, scales=_hashable(a["scales"]), grid=_hashable(a["grid"]))
    return _cached_runner(model, "_ud_spatial_runners", key, lambda: SpatialRunner(model, *a.values()))
