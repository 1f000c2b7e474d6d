"""An adversarial patch: ONE small texture — a sticker, a tattoo, a logo — pasted into every face at a random place, roll and
size, fitted so that it fools the detector wherever it lands: placement_q16, patch_placements, patch_alpha, paste, PatchRunner,
patch_runner and the restatements ref_patch_*.

Every other runner here changes the image a little everywhere (attack.py, universal.py, band.py), at a few pixels per image
(SparseFMNRunner) or moves its pixels (spatial.py, flow.py).  A patch (Brown et al., "Adversarial Patch"; Karmon et al., "LaVAN")
covers a small region, is unbounded inside the clip range there, is one pattern for every image, and has to survive the
placement it cannot choose: expectation over transformation.

The rule (include/unidefense_hip.h states it for the kernels; the ref_* functions below restate it in numpy).
    state      patch [3, P, P] fp32 inside clip; alpha [P, P] fp32 in [0, 1], fixed: "square" all ones, "circle" the disc of
               diameter P with a one-texel linear edge, or an explicit tensor (copied, never aliased)
    placement  per sample a centre (cx, cy) in image pixels, an angle in degrees, a scale s in image pixels per texel,
               0.25 <= s <= 4.  Pixel and texel centres sit on the integers, x to the right, y down; with t0 = (P - 1) / 2 the
               forward map is p = s R(angle) (t - t0) + centre.  placement_q16 makes one row of 16 int32 in float64: the
               inverse map's six Q16 integers floor(v 65536 + 0.5), the forward map's six, reach = floor(s sqrt(2) (1 + 2^-7))
               + 2, three zeros.
    weights    the output pixel (r, c): U = m00 c + m01 r + o0, V likewise, int64; j0 = U >> 16, fx = (U >> 8) & 255, i0 and fy
               from V; taps (i0, j0), (i0, j0 + 1), (i0 + 1, j0), (i0 + 1, j0 + 1) with w = wx wy / 65536, wx in {256 - fx, fx}:
               exact dyadics; omega = fl32(w alpha[i][j]), the only weight either direction uses.  A tap outside the texture,
               or with omega == 0, is absent.
    paste      cov = sum omega, acc = sum omega patch (fp32, tap order, no contraction); out = clamp((1 - cov) x + acc, clip);
               a pixel with no present tap gets x's own bits.
    adjoint    a GATHER, so that a replay gives the same bits: the texel (i, j) of sample n takes the pixel nearest its forward
               image, walks the (2 reach + 1)^2 window around it in row-major order, cut to the image, evaluates the same integer
               inverse map per candidate and accumulates (double) omega (double) g where the candidate names (i, j); rounded once.
    iteration  UniversalRunner's with the paste in place of the add: forward + d/dx at x_adv (pasted with placement row k);
               ud_patch_grad with row k; ud_uap_control (who steers: beta, source; k becomes k + 1); ud_uap_reduce over gp,
               ascending n, fp32; patch <- clamp(patch + step sign(gsum), clip); paste with row k + 1.
The placement table [steps + 1, batch, 16] lives on the device and is refilled per call from a seeded CPU generator outside the
graph (SquareRunner's rule for random choices); row `steps` is the placement x_adv is returned with.  Both kernels read the row
index from a device int, clamped into the table: no host synchronisation in the loop.  The clip's effect on the gradient is
ignored, as everywhere here.
"""
import math

import numpy as np
import torch

from .attack import (_arguments, _cached_runner, _refuse_clip, _refuse_count, _Runner, cross_entropy_each, frozen)
from .universal import _refuse_beta, _refuse_reduce, _refuse_source

ROW = 16                             # int32 words per placement (UD_PATCH_ROW)
MAX_REACH = 8                        # UD_PATCH_MAX_REACH
MAX_P = 256
SCALE_RANGE = (0.25, 4.0)
SHAPES = ("square", "circle")
_I32 = (-(1 << 31), (1 << 31) - 1)


# ---- host side: placements, masks --------------------------------------------------------------------------------------------------
def _refuse_P(P):
    if isinstance(P, bool) or not isinstance(P, (int, np.integer)) or not 1 <= int(P) <= MAX_P:
        raise ValueError(f"patch must be an integer side in [1, {MAX_P}], got {P!r}")


def reach_of(scale):
    """floor(s sqrt(2) (1 + 2^-7)) + 2: how far, in pixels, a pixel that weighs a texel lies from the texel's nearest pixel"""
    return int(math.floor(float(scale) * math.sqrt(2.0) * (1.0 + 2.0 ** -7))) + 2


def placement_q16(P, centre, angle=0.0, scale=1.0):
    """One placement as 16 Python ints (the module's rule): the inverse map (m00, m01, o0, m10, m11, o1: texel column and row
    from pixel column c and row r), the forward map likewise (pixel column and row from texel column j and row i), reach, three
    zeros.  Refused: a scale outside [0.25, 4], anything not finite, an entry that does not fit int32 (a centre 32768 pixels
    away)."""
    _refuse_P(P)
    s, a = float(scale), float(angle)
    if not SCALE_RANGE[0] <= s <= SCALE_RANGE[1]:
        raise ValueError(f"scale must be in [{SCALE_RANGE[0]}, {SCALE_RANGE[1]}] image pixels per texel, got {scale!r}")
    if len(centre) != 2 or not all(math.isfinite(float(v)) for v in centre) or not math.isfinite(a):
        raise ValueError(f"centre must be two finite numbers and angle finite, got {centre!r} and {angle!r}")
    cx, cy = float(centre[0]), float(centre[1])
    co, si = math.cos(math.radians(a)), math.sin(math.radians(a))
    t0 = (int(P) - 1) / 2.0
    f00, f01, f10, f11 = s * co, -s * si, s * si, s * co
    m00, m01, m10, m11 = co / s, si / s, -si / s, co / s
    vals = (m00, m01, t0 - (m00 * cx + m01 * cy), m10, m11, t0 - (m10 * cx + m11 * cy),
            f00, f01, cx - (f00 + f01) * t0, f10, f11, cy - (f10 + f11) * t0)
    row = [int(math.floor(v * 65536.0 + 0.5)) for v in vals] + [reach_of(s), 0, 0, 0]
    if not all(_I32[0] <= v <= _I32[1] for v in row):
        raise ValueError(f"the placement centre={centre!r} angle={angle!r} scale={scale!r} does not fit Q16 in int32")
    return row


def check_table(table):
    """table [..., 16] (numpy or a CPU tensor) as an int32 numpy array; refused before any upload: another shape, a value
    outside int32, reach outside [0, 8], a non-zero reserved word"""
    t = table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
    if t.ndim < 1 or t.shape[-1] != ROW or t.dtype.kind not in "iu":
        raise ValueError(f"a placement table is integers [..., {ROW}], got {t.dtype} {tuple(t.shape)}")
    if t.size and (t.min() < _I32[0] or t.max() > _I32[1]):
        raise ValueError("a placement table holds int32 values")
    if np.any(t[..., 12] < 0) or np.any(t[..., 12] > MAX_REACH):
        raise ValueError(f"a placement's reach must be in [0, {MAX_REACH}], got up to {int(t[..., 12].max())}")
    if np.any(t[..., 13:] != 0):
        raise ValueError("a placement's reserved words must be zero")
    return np.ascontiguousarray(t.astype(np.int32))


def _refuse_placing(P, size, max_angle, scales, region):
    """the arguments of patch_placements: the scale range inside [0.25, 4] and the largest patch's bounding circle inside region"""
    _refuse_P(P)
    if not (math.isfinite(float(max_angle)) and 0.0 <= float(max_angle) <= 180.0):
        raise ValueError(f"max_angle must be in [0, 180] degrees, got {max_angle!r}")
    if len(scales) != 2 or not SCALE_RANGE[0] <= float(scales[0]) <= float(scales[1]) <= SCALE_RANGE[1]:
        raise ValueError(f"scales must be (lo, hi) with {SCALE_RANGE[0]} <= lo <= hi <= {SCALE_RANGE[1]}, got {scales!r}")
    if len(region) != 4 or not (0.0 <= float(region[0]) < float(region[2]) <= 1.0 and 0.0 <= float(region[1]) < float(region[3]) <= 1.0):
        raise ValueError(f"region must be (x0, y0, x1, y1) fractions of the image with 0 <= x0 < x1 <= 1 and 0 <= y0 < y1 <= 1, got {region!r}")
    radius = float(scales[1]) * int(P) / math.sqrt(2.0)
    side = min(float(region[2]) - float(region[0]), float(region[3]) - float(region[1])) * int(size)
    if 2.0 * radius > side:
        raise ValueError(f"a patch of side {int(P)} at scale {float(scales[1])} (bounding circle of radius {radius:.1f} pixels) does "
                         f"not fit the region {tuple(region)!r} of a {int(size)}-pixel image")


def patch_placements(n, size, patch, max_angle=15.0, scales=(0.8, 1.25), region=(0.0, 0.0, 1.0, 1.0), generator=None):
    """n random placements of a patch of side `patch` in a size-pixel image: (params float64 [n, 4]: cx, cy, angle, scale; table
    int32 [n, 16]), CPU tensors.  Drawn from `generator` (a CPU torch.Generator; None: the global one) as ONE torch.rand(n, 4)
    in float64: the scale uniform in `scales`, the angle uniform in +-max_angle, the centre uniform where the patch's bounding
    circle (radius s P / sqrt(2)) stays inside `region`, (x0, y0, x1, y1) as fractions of the image.  Refused if it cannot."""
    _refuse_count("n", n, 1)
    _refuse_placing(patch, size, max_angle, scales, region)
    u = torch.rand(int(n), 4, dtype=torch.float64, generator=generator).numpy()
    s = float(scales[0]) + u[:, 3] * (float(scales[1]) - float(scales[0]))
    ang = (2.0 * u[:, 2] - 1.0) * float(max_angle)
    rad = s * int(patch) / math.sqrt(2.0)
    x0, y0, x1, y1 = (float(v) * int(size) - 0.5 for v in region)          # the region's edges in pixel coordinates
    cx = x0 + rad + u[:, 0] * (x1 - x0 - 2.0 * rad)
    cy = y0 + rad + u[:, 1] * (y1 - y0 - 2.0 * rad)
    params = np.stack([cx, cy, ang, s], 1)
    table = np.array([placement_q16(patch, (p[0], p[1]), p[2], p[3]) for p in params], dtype=np.int32)
    return torch.from_numpy(params), torch.from_numpy(table)


def patch_alpha(P, shape="square"):
    """The coverage mask [P, P] fp32: "square" all ones; "circle" clamp(P / 2 + 1 / 2 - d, 0, 1) with d the texel centre's
    distance from the patch centre: the disc of diameter P, its edge a linear ramp one texel wide"""
    _refuse_P(P)
    if shape not in SHAPES:
        raise ValueError(f"shape must be one of {SHAPES}, got {shape!r}")
    P = int(P)
    if shape == "square":
        return torch.ones(P, P, dtype=torch.float32)
    t = torch.arange(P, dtype=torch.float64) - (P - 1) / 2.0
    d = torch.sqrt(t[:, None] ** 2 + t[None, :] ** 2)
    return (P / 2.0 + 0.5 - d).clamp_(0.0, 1.0).to(torch.float32)


def _alpha_for(alpha, shape, P):
    if alpha is None:
        return patch_alpha(P, shape)
    if not isinstance(alpha, torch.Tensor) or tuple(alpha.shape) != (P, P):
        raise ValueError(f"alpha must be a [{P}, {P}] tensor, got {tuple(alpha.shape) if isinstance(alpha, torch.Tensor) else type(alpha).__name__}")
    a = alpha.detach().to(device="cpu", dtype=torch.float32)
    if not bool(((a >= 0.0) & (a <= 1.0)).all()):
        raise ValueError("alpha must lie in [0, 1]")
    return a.clone()


def paste(x, patch, table, alpha=None, clip=(-1.0, 1.0), out=None):
    """x [n, 3, S, S] cuda fp32 with patch [3, P, P] pasted into sample i under the placement table[i] (int [n, 16], as
    patch_placements returns it: checked on the host, then uploaded); alpha [P, P] (None: all ones); a new tensor, or `out`
    (like x, not x).  One launch (ud_patch_paste)."""
    from . import kernels as K
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError("paste takes a cuda fp32 [n, 3, S, S] batch")
    if not isinstance(patch, torch.Tensor) or patch.dim() != 3 or patch.shape[0] != 3 or patch.shape[1] != patch.shape[2]:
        raise ValueError(f"a patch is a [3, P, P] tensor, got {tuple(patch.shape) if isinstance(patch, torch.Tensor) else type(patch).__name__}")
    _refuse_clip(clip)
    P = int(patch.shape[1])
    _refuse_P(P)
    t = check_table(table)
    if t.shape != (x.shape[0], ROW):
        raise ValueError(f"table must be [{x.shape[0]}, {ROW}], one placement per sample, got {tuple(t.shape)}")
    dev = x.device
    a = _alpha_for(alpha, "square", P).to(dev)
    src = x.detach().contiguous()
    if out is None:
        out = torch.empty_like(src)
    elif out.shape != x.shape or out.dtype != x.dtype or out.device != dev or not out.is_contiguous():
        raise ValueError("out must be a contiguous tensor like x")
    tab = torch.from_numpy(t).view(1, -1, ROW).to(dev)
    k = torch.zeros(1, dtype=torch.int32, device=dev)
    return K.patch_paste(src, patch.detach().to(device=dev, dtype=torch.float32).contiguous(), a, tab, k, out, float(clip[0]), float(clip[1]))


# ---- numpy restatements of the three kernels' rules (tests compare the GPU with these) -------------------------------------------
def _np(a, dtype):
    return np.ascontiguousarray((a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(dtype))


def _weight(fx, fy, dj, di):
    return np.where(dj != 0, fx, 256 - fx) * np.where(di != 0, fy, 256 - fy)


def _omega(wi, a):
    """fl32(w alpha): w = wi / 65536 exact in float32, one rounding for the product"""
    return (wi.astype(np.float32) * np.float32(1.0 / 65536.0)) * a.astype(np.float32)


def ref_patch_taps(row, alpha, S):
    """the four taps of every pixel of an S x S image under the placement `row`: a list of (i, j, omega, present), each [S, S]
    (i, j int64 and clipped into the texture where the tap is absent; omega float32)"""
    alpha = _np(alpha, np.float32)
    P = alpha.shape[0]
    m = [int(v) for v in row[:6]]
    r, c = np.meshgrid(np.arange(S, dtype=np.int64), np.arange(S, dtype=np.int64), indexing="ij")
    U, V = m[0] * c + m[1] * r + m[2], m[3] * c + m[4] * r + m[5]
    j0, i0, fx, fy = U >> 16, V >> 16, (U >> 8) & 255, (V >> 8) & 255
    taps = []
    for t in range(4):
        di, dj = t >> 1, t & 1
        i, j = i0 + di, j0 + dj
        inside = (i >= 0) & (i <= P - 1) & (j >= 0) & (j <= P - 1)
        i, j = np.clip(i, 0, P - 1), np.clip(j, 0, P - 1)
        om = _omega(_weight(fx, fy, dj, di), alpha[i, j])
        taps.append((i, j, om, inside & (om != 0)))
    return taps


def ref_patch_paste(x, patch, alpha, table, lo=-1.0, hi=1.0):
    """ud_patch_paste in numpy float32, bit for bit: x [N, 3, S, S], patch [3, P, P], alpha [P, P], table [N, 16]"""
    x, patch = _np(x, np.float32), _np(patch, np.float32)
    table = check_table(table)
    lo, hi = np.float32(lo), np.float32(hi)
    out = x.copy()
    with np.errstate(invalid="ignore"):
        for n in range(x.shape[0]):
            cov = np.zeros(x.shape[2:], np.float32)
            acc = np.zeros(x.shape[1:], np.float32)
            some = np.zeros(x.shape[2:], bool)
            for i, j, om, present in ref_patch_taps(table[n], alpha, x.shape[2]):
                some |= present
                cov = np.where(present, cov + om, cov)
                acc = np.where(present, acc + om * patch[:, i, j], acc)
            v = (np.float32(1.0) - cov) * x[n] + acc
            v = np.where(v < lo, lo, v)
            v = np.where(v > hi, hi, v)
            out[n] = np.where(some & (cov != 0), v, x[n])
    return out


def ref_patch_grad(g, alpha, table, magnitude=False):
    """The adjoint of the paste with respect to the patch, per sample, as a float64 SCATTER over every pixel of the image (no
    window): gp [N, 3, P, P] float64.  magnitude=True: also sum |omega g| per element, the scale of the gather's rounding."""
    g, alpha = _np(g, np.float64), _np(alpha, np.float32)
    table = check_table(table)
    P = alpha.shape[0]
    out, mag = np.zeros((g.shape[0], 3, P, P)), np.zeros((g.shape[0], 3, P, P))
    for n in range(g.shape[0]):
        for i, j, om, present in ref_patch_taps(table[n], alpha, g.shape[2]):
            ii, jj, w = i[present], j[present], om[present].astype(np.float64)
            for ch in range(3):
                term = w * g[n, ch][present]
                np.add.at(out[n, ch], (ii, jj), term)
                np.add.at(mag[n, ch], (ii, jj), np.abs(term))
    return (out, mag) if magnitude else out


def ref_patch_grad_gather(g, alpha, table, shrink=0):
    """ud_patch_grad's own walk in numpy: per texel the window of reach - shrink around the nearest pixel of its forward image,
    row-major, sums in float64 rounded once to float32 [N, 3, P, P].  shrink > 0 shows what a smaller window loses."""
    g, alpha = _np(g, np.float32), _np(alpha, np.float32)
    table = check_table(table)
    N, S, P = g.shape[0], g.shape[2], alpha.shape[0]
    i, j = np.meshgrid(np.arange(P, dtype=np.int64), np.arange(P, dtype=np.int64), indexing="ij")
    out = np.zeros((N, 3, P, P), np.float32)
    for n in range(N):
        m = [int(v) for v in table[n]]
        pc, pr = (m[6] * j + m[7] * i + m[8] + 32768) >> 16, (m[9] * j + m[10] * i + m[11] + 32768) >> 16
        reach = max(min(max(m[12], 0), MAX_REACH) - int(shrink), 0)
        acc = np.zeros((3, P, P))
        for dr in range(-reach, reach + 1):
            for dc in range(-reach, reach + 1):
                r, c = pr + dr, pc + dc
                ok = (r >= 0) & (r <= S - 1) & (c >= 0) & (c <= S - 1)
                U, V = m[0] * c + m[1] * r + m[2], m[3] * c + m[4] * r + m[5]
                dj, di = j - (U >> 16), i - (V >> 16)
                ok &= (dj >= 0) & (dj <= 1) & (di >= 0) & (di <= 1)
                om = _omega(_weight((U >> 8) & 255, (V >> 8) & 255, dj, di), alpha)
                ok &= om != 0
                rr, cc = np.clip(r, 0, S - 1), np.clip(c, 0, S - 1)
                acc += np.where(ok, om.astype(np.float64) * g[n][:, rr, cc].astype(np.float64), 0.0)
        out[n] = acc.astype(np.float32)
    return out


def ref_patch_update(patch, gsum, step, lo=-1.0, hi=1.0):
    """clamp(patch + step sign(gsum), lo, hi) in float64, sign(0) = 0, a NaN kept"""
    patch, gsum = _np(patch, np.float64), _np(gsum, np.float64)
    with np.errstate(invalid="ignore"):
        v = patch + float(step) * np.sign(gsum)
        v = np.where(v < lo, float(lo), v)
        return np.where(v > hi, float(hi), v)


def ref_patch_fit(grad, x, patch, alpha, tables, step, clip=(-1.0, 1.0), beta=math.inf, source=None, y=None):
    """The whole loop on a callable gradient: grad(x_adv float32 [N, 3, S, S]) -> (g [N, 3, S, S], f [N]); tables [steps + 1, N,
    16].  Per iteration k: paste with row k, g and f there, the scatter adjoint, who steers (f < beta, y == source), their sum
    in ascending n in float64, the signed step inside clip.  Returns (patch float64, x_adv pasted with the last row)."""
    tables = check_table(tables)
    lo, hi = float(clip[0]), float(clip[1])
    patch = _np(patch, np.float64)
    for k in range(tables.shape[0] - 1):
        g, f = grad(ref_patch_paste(x, patch, alpha, tables[k], lo, hi))
        gp = ref_patch_grad(g, alpha, tables[k])
        w = _np(f, np.float64) < float(beta)
        if source is not None:
            w &= _np(y, np.int64) == int(source)
        gsum = np.zeros_like(patch)
        for n in range(gp.shape[0]):
            if w[n]:
                gsum = gsum + gp[n]
        patch = ref_patch_update(patch, gsum, step, lo, hi)
    return patch, ref_patch_paste(x, patch, alpha, tables[-1], lo, hi)


# ---- the runner ---------------------------------------------------------------------------------------------------------------------
def resolve_patch_step(clip, step=None):
    """step=None: (hi - lo) / 64"""
    return (float(clip[1]) - float(clip[0])) / 64.0 if step is None else float(step)


class PatchRunner(_Runner):
    """runner = PatchRunner(model, batch, size, patch=32, ...); x_adv = runner(x, y, generator=None).

    `steps` iterations of the module's rule on the batch (x, y), STARTING FROM THE patch THE RUNNER HOLDS (a fresh runner, or
    reset(): zeros), each at freshly drawn placements; returns x_adv, the batch with the new patch pasted at the call's last
    row of placements, a static buffer.  patch [3, P, P] fp32 persists across calls: a fit is a loop of calls over batches and
    epochs.  shape / alpha: the coverage mask (patch_alpha; an explicit alpha is copied).  max_angle, scales, region:
    patch_placements' ranges.  step=None: (hi - lo) / 64.  beta, source, reduce, precision, grad_scale: as UniversalRunner.
    generator: a CPU torch.Generator for the placements (None: the global one), consumed outside the graph.
    reduce=None: one hipGraph holds the iteration — _grad, ud_patch_grad, ud_uap_control, ud_uap_reduce, ud_patch_update,
    ud_patch_paste.  reduce=callable: two graphs with reduce(gsum) between them, the data-parallel hook.
    apply(x, generator=None, table=None) pastes the patch into any [n, 3, size, size] batch, no backward.

    history [steps, batch], counted [steps, batch] int32, placements [steps + 1, batch, 4] float64 (cx, cy, angle, scale) hold
    the LAST call's values; g, gp, gsum, out: static buffers; args: the resolved arguments with `area`, the nominal share
    P^2 mean(s)^2 / size^2 of the image."""
    _what = "PatchRunner"

    def __init__(self, model, batch, size, patch=32, shape="square", alpha=None, steps=1, step=None, max_angle=15.0,
                 scales=(0.8, 1.25), region=(0.0, 0.0, 1.0, 1.0), beta=math.inf, source=None, clip=(-1.0, 1.0), precision="fp32",
                 grad_scale=None, reduce=None):
        _refuse_count("steps", steps, 1)
        _refuse_clip(clip)
        _refuse_placing(patch, size, max_angle, scales, region)
        if shape not in SHAPES:
            raise ValueError(f"shape must be one of {SHAPES}, got {shape!r}")
        mask = _alpha_for(alpha, shape, int(patch))
        _refuse_beta(beta)
        _refuse_source(source)
        _refuse_reduce(reduce)
        if step is not None and not math.isfinite(float(step)):
            raise ValueError(f"step must be finite, got {step!r}")
        self._init_model(model, batch, size, precision, lambda: self._init_loss("cross_entropy", grad_scale))
        self.objective = cross_entropy_each
        self.P, self.steps, self.lo, self.hi = int(patch), int(steps), float(clip[0]), float(clip[1])
        self.step = resolve_patch_step(clip, step)
        self.max_angle, self.scales, self.region = float(max_angle), tuple(map(float, scales)), tuple(map(float, region))
        self.beta, self.source, self.reduce = float(beta), None if source is None else int(source), reduce
        self.args = {"method": "patch", "patch": self.P, "shape": "given" if alpha is not None else shape, "steps": self.steps,
                     "step": self.step, "max_angle": self.max_angle, "scales": self.scales, "region": self.region,
                     "beta": self.beta, "source": self.source, "clip": (self.lo, self.hi), "precision": self.precision,
                     "grad_scale": self.grad_scale, "reduce": None if reduce is None else getattr(reduce, "__name__", repr(reduce)),
                     "area": self.P ** 2 * (0.5 * (self.scales[0] + self.scales[1])) ** 2 / float(self.size) ** 2}
        self.alpha = mask.to(self.device)                         # the runner's own: the given tensor is never aliased
        self.patch = torch.zeros(3, self.P, self.P, dtype=torch.float32, device=self.device)
        self.update_graph = None
        self.x0 = self.x_adv = self.y = self.history = self.counted = self.gsum = self.gp = self.table = self.placements = None

    def reset(self, value=0.0):
        """the patch back to a constant (0.0: mid-grey for the default clip) or to a [3, P, P] tensor, clamped into clip"""
        with torch.no_grad():
            if isinstance(value, torch.Tensor):
                if tuple(value.shape) != tuple(self.patch.shape):
                    raise ValueError(f"a patch is [3, {self.P}, {self.P}], got {tuple(value.shape)}")
                self.patch.copy_(value.detach().to(torch.float32))
            else:
                self.patch.fill_(float(value))
            self.patch.clamp_(self.lo, self.hi)

    def draw(self, n, generator=None):
        """n placements from the runner's ranges: patch_placements' (params, table)"""
        return patch_placements(n, self.size, self.P, self.max_angle, self.scales, self.region, generator)

    def _buffers(self, x, y):
        from . import kernels as K
        dev = self.device
        self.x0 = x.detach().clone().contiguous()
        self.x_adv = torch.empty_like(self.x0).requires_grad_()   # the static leaf: x0 with the patch pasted
        self.y = y.detach().clone()
        self.ist, self.w, self.history, self.counted = K.uap_state(self.batch, self.steps, dev)
        self.gsum = torch.zeros_like(self.patch)
        self.gp = torch.zeros(self.batch, 3, self.P, self.P, dtype=torch.float32, device=dev)
        self.table = torch.zeros(self.steps + 1, self.batch, ROW, dtype=torch.int32, device=dev)

    def _paste(self):
        from . import kernels as K
        with torch.no_grad():
            K.patch_paste(self.x0, self.patch, self.alpha, self.table, self.ist, self.x_adv, self.lo, self.hi)

    def _gradient(self):
        """forward + d/dx at x_adv, its adjoint onto the patch per sample, who steers, their sum: up to the reduce hook"""
        from . import kernels as K
        g, self.out, f = self._grad(self.x_adv, self._each)
        self.g = g = g.contiguous()
        K.patch_grad(g, self.alpha, self.table, self.ist, self.gp)          # row k: the counter is still this iteration's
        K.uap_control(f.detach().float().contiguous(), self.y, self.w, self.ist, self.history, self.counted, self.beta, self.source)
        K.uap_reduce(self.gp, self.w, self.gsum)

    def _update(self):
        """the patch's step from gsum and the new x_adv at the next row of placements"""
        from . import kernels as K
        K.patch_update(self.patch, self.gsum, self.step, self.lo, self.hi)
        self._paste()                                             # row k + 1: the control has advanced the counter

    def _iteration(self):
        """one iteration on the static buffers: what the single graph holds"""
        self._gradient()
        self._update()

    def _start(self, x, y, generator):
        params, table = self.draw((self.steps + 1) * self.batch, generator)
        self.placements = params.view(self.steps + 1, self.batch, 4)
        with torch.no_grad():
            self.x0.copy_(x)
            self.y.copy_(y)
            self.table.copy_(torch.from_numpy(check_table(table)).view(self.steps + 1, self.batch, ROW))
            self.ist.zero_()                                      # every row of history and counted is written again
        self._paste()

    def __call__(self, x, y, generator=None):
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
            self._start(x, y, generator)
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
    def apply(self, x, generator=None, table=None):
        """x (cuda fp32 [n, 3, size, size], any n) with the patch pasted at `table` ([n, 16], as draw() returns it) or at n
        placements drawn from `generator`: a new tensor"""
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError(f"{self._what}.apply takes a cuda tensor")
        if x.dim() != 4 or x.shape[0] < 1 or tuple(x.shape[1:]) != self.shape[1:] or x.dtype != torch.float32:
            raise ValueError(f"input {tuple(x.shape)} {x.dtype} is no [n, {', '.join(map(str, self.shape[1:]))}] torch.float32 batch")
        if table is None:
            table = self.draw(x.shape[0], generator)[1]
        return paste(x, self.patch, table, self.alpha, (self.lo, self.hi))


_patch_arguments = _arguments(PatchRunner)


def _patch_keyed(a):
    """the bound arguments in their hashable form: an explicit alpha only as the fact that there is one (contents, which the
    runner copies), a callable reduce by identity, the ranges as tuples"""
    return dict(a, alpha=a["alpha"] is not None, reduce=None if a["reduce"] is None else id(a["reduce"]),
                scales=tuple(a["scales"]), region=tuple(a["region"]))


def patch_runner(model, *args, **kwargs):
    """The model's PatchRunner for the full argument tuple (PatchRunner's after the model), made on first use; at most
    _MAX_RUNNERS are kept, in a dictionary of their own.  The runner holds the patch: the same arguments give the same patch
    back.  With an explicit `alpha` the other arguments are the key, and every fetch copies the given alpha into the runner."""
    a = _patch_arguments(*args, **kwargs)
    made = []
    r = _cached_runner(model, "_ud_patch_runners", _patch_keyed(a), lambda: made.append(1) or PatchRunner(model, *a.values()))
    if a["alpha"] is not None and not made:
        r.alpha.copy_(_alpha_for(a["alpha"], "square", r.P))
    return r
