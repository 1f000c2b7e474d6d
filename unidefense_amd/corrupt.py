"""Common image corruptions on the device: corrupt() and CorruptionRunner.

What happens to a frame between the forger and the detector — recompression, blur, noise, down-sampling, colour shifts, dropped
blocks — as seven corruptions at five severities each (LEVELS), applied to the normalised fp32 batch where it lives.  All of
them are defined on 8-bit grey levels with integer arithmetic (csrc/corrupt.hip, include/unidefense_hip.h): a model input x in
[-1, 1] is read as the level clamp(floor((x + 1) 127.5 + 0.5), 0, 255), the corruption maps levels to levels, and the result is
written through a 256-entry table (level_table).  The table's values quantise back to 0..255, so a chain of corruptions is
exactly the composition of its stages, and tests/test_corrupt_cpu.py restates every kernel in numpy bit for bit.  Every
corruption is one launch that reads the batch once and writes it once.

Every table a kernel reads (levels, JPEG quantisation tables, blur taps) is made here on the host, in integers or float64, and
every random choice (the noise field, the block positions) is drawn by torch outside any captured graph.

corrupt(x, kind, ...) is the functional form on any cuda fp32 [N, 3, S, S] tensor.  CorruptionRunner follows the attack runners'
life cycle (unidefense_amd/attack.py: _Runner): call 1 runs eagerly, call 2 captures the corruption launches followed by the eval
forward (InferenceRunner's, in either precision) into one hipGraph, later calls copy the input in, refill the random tables and
replay.  No tape, no gradient, nothing frozen.
"""
import math

import torch

from .attack import _Runner, _arguments, _cached_runner, _detached
from .infer import _check_precision, _eval_nodes

CORRUPTIONS = ("jpeg", "gaussian_blur", "gaussian_noise", "pixelate", "contrast", "saturation", "block")
LEVELS = {
    "jpeg": (90, 70, 50, 30, 10),                           # quality
    "gaussian_blur": (7, 9, 13, 17, 21),                    # kernel size; sigma = 0.3 ((k - 1) / 2 - 1) + 0.8
    "gaussian_noise": (0.001, 0.002, 0.005, 0.01, 0.05),    # variance on the [0, 1] scale
    "pixelate": (2, 3, 4, 5, 6),                            # cell side
    "contrast": (0.85, 0.725, 0.6, 0.475, 0.35),            # factor about level 128
    "saturation": (0.4, 0.3, 0.2, 0.1, 0.0),                # chroma factor
    "block": (16, 32, 48, 64, 80),                          # 8 x 8 blocks at level 128
}
SUBSAMPLINGS = ("420", "444")
BLUR_MAX_K, PIXELATE_MAX, BLOCK_MAX = 31, 256, 1024        # what the kernels take (include/unidefense_hip.h)

# Annex K of the JPEG standard, row-major natural order
JPEG_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
             14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
             49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
JPEG_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
               47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32


# ---- host tables: integers and float64 only, the same on any machine -------------------------------------------------------------
def level_table():
    """[256] float64: level / 127.5 - 1; rounded once to fp32 it is what the kernels write"""
    return [level / 127.5 - 1.0 for level in range(256)]


def jpeg_scale(quality):
    q = int(quality)
    return 5000 // q if q < 50 else 200 - 2 * q


def jpeg_tables(quality):
    """(luma, chroma): the Annex-K tables at `quality` by the standard rule, 64 ints each in 1..255"""
    s = jpeg_scale(quality)
    return tuple(tuple(min(max((b * s + 50) // 100, 1), 255) for b in base) for base in (JPEG_LUMA, JPEG_CHROMA))


def dct_table():
    """T[k][n] = round(c_k cos((2n + 1) k pi / 16) 2^13), c_0 = sqrt(1/8), c_k = 1/2"""
    return tuple(tuple(int(math.floor((math.sqrt(0.125) if k == 0 else 0.5) * math.cos((2 * n + 1) * k * math.pi / 16.0)
                                      * 8192.0 + 0.5)) for n in range(8)) for k in range(8))


def blur_sigma(k):
    return 0.3 * ((int(k) - 1) / 2.0 - 1.0) + 0.8


def blur_weights(k):
    """k integer taps that sum to exactly 2^14: round(g 2^14) of the normalised Gaussian, the centre absorbing the remainder"""
    k = int(k)
    r, sigma = k // 2, blur_sigma(k)
    g = [math.exp(-((i - r) ** 2) / (2.0 * sigma * sigma)) for i in range(k)]
    total = sum(g)
    w = [int(math.floor(v / total * 16384.0 + 0.5)) for v in g]
    w[r] += 16384 - sum(w)
    return tuple(w)


def noise_scale(var):
    """s = 255 sqrt(var), rounded once to fp32: the factor on z in level units"""
    return float(torch.tensor(255.0 * math.sqrt(float(var)), dtype=torch.float64).to(torch.float32))


def q8(factor):
    return int(math.floor(256.0 * float(factor) + 0.5))


# ---- arguments ---------------------------------------------------------------------------------------------------------------------
def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _param(kind, v):
    """a stage's parameter in the form its kernel takes, refused where the kernel would refuse it"""
    if kind in ("jpeg", "gaussian_blur", "pixelate", "block"):
        lo, hi = {"jpeg": (1, 100), "gaussian_blur": (1, BLUR_MAX_K), "pixelate": (1, PIXELATE_MAX), "block": (0, BLOCK_MAX)}[kind]
        if not _is_int(v) or not lo <= v <= hi or (kind == "gaussian_blur" and v % 2 == 0):
            raise ValueError(f"{kind} takes an {'odd ' if kind == 'gaussian_blur' else ''}integer in {lo}..{hi}, got {v!r}")
        return v
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= float(v) <= (1.0 if kind == "gaussian_noise" else 256.0):
        raise ValueError(f"{kind} takes a number >= 0 (a variance <= 1, a factor <= 256), got {v!r}")
    return float(v)


def _stage(kind, level, param):
    if kind not in CORRUPTIONS:
        raise ValueError(f"corruption must be one of {CORRUPTIONS}, got {kind!r}")
    if param is not None:
        return kind, _param(kind, param)
    if level is None:
        raise ValueError(f"{kind} needs a level 1..5 or a param")
    if not _is_int(level) or not 1 <= level <= 5:
        raise ValueError(f"level must be an integer 1..5, got {level!r}")
    return kind, LEVELS[kind][level - 1]


def resolve(kind, level=None, param=None):
    """The stages of a corruption as a tuple of (name, parameter) pairs, in the order they are applied.  kind: one name with a
    level 1..5 (LEVELS) or an explicit param that overrides it; or a list of (name, level) / (name, {"level": l}) /
    (name, {"param": v}) pairs, e.g. [("gaussian_blur", 3), ("jpeg", 4)]: blur, then JPEG."""
    if isinstance(kind, str):
        return (_stage(kind, level, param),)
    if not isinstance(kind, (list, tuple)) or not kind:
        raise ValueError(f"corruption must be one of {CORRUPTIONS} or a list of (name, level) pairs, got {kind!r}")
    stages = []
    for pair in kind:
        if not isinstance(pair, (list, tuple)) or len(pair) != 2 or not isinstance(pair[0], str):
            raise ValueError(f"a chain is a list of (name, level) or (name, {{'param': value}}) pairs, got {pair!r}")
        name, what = pair
        if isinstance(what, dict):
            if set(what) - {"level", "param"} or len(what) != 1:
                raise ValueError(f"a pair takes exactly one of 'level' and 'param', got {what!r}")
            stages.append(_stage(name, what.get("level"), what.get("param")))
        else:
            stages.append(_stage(name, what, None))
    return tuple(stages)


def _refuse_subsampling(subsampling):
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"subsampling must be one of {SUBSAMPLINGS}, got {subsampling!r}")


def _refuse_size(stages, size):
    for kind, p in stages:
        if kind == "gaussian_blur" and size < (p + 1) // 2:
            raise ValueError(f"a {p}-tap blur reflects up to {p // 2} pixels: size must be >= {(p + 1) // 2}, got {size}")


# ---- device tables and draws -------------------------------------------------------------------------------------------------------
_tables = {}            # (device, what) -> tensor: made once, read by eager launches and captured graphs alike


def _table(device, what, make, dtype):
    key = (str(device), what)
    if key not in _tables:
        _tables[key] = torch.tensor(make(), dtype=torch.float64 if dtype == torch.float32 else torch.int64).to(dtype).to(device)
    return _tables[key]


def _lut(device):
    return _table(device, "levels", level_table, torch.float32)


def draw_noise(shape, generator, device):
    """z ~ N(0, 1) of the batch's shape, on the generator's device (None: `device`'s default generator)"""
    gdev = generator.device if generator is not None else device
    return torch.randn(tuple(shape), generator=generator, device=gdev, dtype=torch.float32).to(device)


def draw_blocks(batch, count, size, generator, device):
    """[batch, count, 2] int32 (row, column) of each block's first pixel, uniform on -7 .. size - 1: blocks may hang over any
    edge and are clipped there"""
    gdev = generator.device if generator is not None else device
    return torch.randint(-7, int(size), (int(batch), int(count), 2), generator=generator, device=gdev).to(torch.int32).to(device)


def _launch(stage, src, dst, subsampling, extra):
    """one stage, one launch: dst = stage(src); extra: the stage's random table (noise: z, block: pos)"""
    from . import kernels as K
    kind, p = stage
    dev = src.device
    lut = _lut(dev)
    if kind == "jpeg":
        qt = _table(dev, ("jpeg", p), lambda: sum(jpeg_tables(p), ()), torch.int32)
        K.corrupt_jpeg(src, dst, lut, qt, p, subsampling)
    elif kind == "gaussian_blur":
        K.corrupt_blur(src, dst, lut, _table(dev, ("blur", p), lambda: blur_weights(p), torch.int32))
    elif kind == "gaussian_noise":
        K.corrupt_point(src, dst, lut, kind, s=noise_scale(p), z=extra)
    elif kind == "pixelate":
        K.corrupt_pixelate(src, dst, lut, p)
    elif kind == "block":
        K.corrupt_blocks(src, dst, lut, extra)
    else:
        K.corrupt_point(src, dst, lut, kind, f8=q8(p))
    return dst


def _draw(stage, shape, generator, device):
    kind, p = stage
    if kind == "gaussian_noise":
        return draw_noise(shape, generator, device)
    if kind == "block":
        return draw_blocks(shape[0], p, shape[2], generator, device)
    return None


def _check_images(x, what):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError(f"{what} takes a cuda tensor")
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3] or x.dtype != torch.float32:
        raise ValueError(f"{what} takes fp32 [N, 3, size, size] images, got {tuple(x.shape)} {x.dtype}")


@torch.no_grad()
def corrupt(x, kind, level=3, param=None, generator=None, subsampling="420", out=None):
    """x corrupted: a new tensor (or `out`, which must not be x) like x, a cuda fp32 [N, 3, S, S] batch in model units.
    kind, level, param: see resolve (a chain applies its stages in order; the random stages draw from `generator` in that
    order).  subsampling: JPEG's chroma format, "420" or "444".  One launch per stage; x is not changed."""
    stages = resolve(kind, level, param)
    _refuse_subsampling(subsampling)
    _check_images(x, "corrupt")
    _refuse_size(stages, x.shape[2])
    if out is not None and (out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous()
                            or out.data_ptr() == x.data_ptr()):
        raise ValueError("out must be a contiguous tensor like x and not x itself")
    src = x.detach().contiguous()
    out = torch.empty_like(src) if out is None else out
    spare = torch.empty_like(src) if len(stages) > 1 else None
    for i, stage in enumerate(stages):
        dst = out if (len(stages) - 1 - i) % 2 == 0 else spare          # the last stage lands in out
        src = _launch(stage, src, dst, subsampling, _draw(stage, x.shape, generator, x.device))
    return out


class CorruptionRunner(_Runner):
    """runner = CorruptionRunner(model, batch, size, kind, level=3, ...); out = runner(x[, generator]).

    The corruption (kind, level, param: see resolve; subsampling: JPEG's) in front of the eval forward, as one hipGraph: the
    stages' launches, then the forward InferenceRunner replays (precision "fp32", or "fp16" on UDEB4), under no_grad.  Returns the
    forward's output dict in static buffers that the next call overwrites; x_cor is the corrupted batch the forward saw (bitwise
    corrupt(x, ...) with the same draws) and args the resolved arguments.  gaussian_noise and block refill their device tables
    from `generator` (draw_noise, draw_blocks; None: the device's default generator) before every call, outside the graph."""
    _what = "CorruptionRunner"
    _backward = False

    def __init__(self, model, batch, size, kind, level=3, param=None, precision="fp32", subsampling="420"):
        def arguments():
            self.stages = resolve(kind, level, param)
            _refuse_subsampling(subsampling)
            _refuse_size(self.stages, int(size))
        self._init_model(model, batch, size, precision, arguments)
        self.subsampling = subsampling
        self.args = {"corruption": self.stages, "subsampling": subsampling, "precision": precision}
        self.x = self.x_cor = None

    def _check(self, x):
        _check_images(x, self._what)
        if tuple(x.shape) != self.shape:
            raise ValueError(f"input {tuple(x.shape)} differs from the runner's key {self.shape}")
        if self.model.training:
            raise ValueError("the model is in training mode: call model.eval() before the runner")

    def _buffers(self, x):
        self.x = x.detach().clone().contiguous()
        self._bufs = [torch.zeros_like(self.x) for _ in self.stages]
        self._extra = [_draw(stage, self.shape, None, self.device) for stage in self.stages]
        self.x_cor = self._bufs[-1]

    def _iteration(self):
        """what the graph holds: one launch per stage on the static buffers, then the forward"""
        src = self.x
        for stage, dst, extra in zip(self.stages, self._bufs, self._extra):
            src = _launch(stage, src, dst, self.subsampling, extra)
        with torch.no_grad(), _eval_nodes(self.model, self.half):
            self.out = _detached(self.model(self.x_cor))

    def __call__(self, x, generator=None):
        self._check(x)
        self.calls += 1
        if self.calls == 1:
            self._buffers(x)
        elif self.graph is None:
            self.graph, = self._capture(self._iteration)
        with torch.no_grad():
            self.x.copy_(x)
            for stage, extra in zip(self.stages, self._extra):
                if extra is not None:
                    extra.copy_(_draw(stage, self.shape, generator, self.device))
        if self.graph is None:
            self._iteration()
        else:
            self.graph.replay()
        return self.out


_corruption_arguments = _arguments(CorruptionRunner)


def _hashable(v):
    if isinstance(v, dict):
        return tuple(sorted((k, _hashable(w)) for k, w in v.items()))
    if isinstance(v, (list, tuple)):
        return tuple(_hashable(w) for w in v)
    return v


def corruption_runner(model, *args, **kwargs):
    """The model's CorruptionRunner for the full argument tuple (CorruptionRunner's after the model), made on first use; at most
    four are kept, in a dictionary of their own (the other runners' caches are untouched)."""
    a = _corruption_arguments(*args, **kwargs)
    _check_precision(model, a["precision"])
    key = dict(a, kind=_hashable(a["kind"]), param=_hashable(a["param"]))
    return _cached_runner(model, "_ud_corruption_runners", key, lambda: CorruptionRunner(model, *a.values()))
