"""CPU: the image corruptions of unidefense_amd/corrupt.py restated in numpy (int64 / float32), their host tables, exact cases,
JPEG against PIL, monotone severities, refusals.  ref_quantise, ref_jpeg, ref_blur, ref_point, ref_pixelate and ref_blocks are
the definition the kernels of csrc/corrupt.hip are held to bit for bit (tests/test_p_corrupt_gpu.py).

A note on the constant-image case: a JPEG keeps a constant block only up to its DC step (Q_dc / 8 levels: 10 levels at quality
10), whatever the arithmetic.  The case is therefore run on the constants every quality can represent — level 128 and
128 +- Q_dc — to within one level (the colour transform's rounding), and on arbitrary constants to within half a DC step of
luma and chroma plus that one level, the bound an exact JPEG meets too.
"""
import io
import math

import numpy as np
import pytest

from unidefense_amd import corrupt as CR


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def ref_quantise(x):
    """levels (int64) of model units x: clamp(floor((x + 1) 127.5 + 0.5), 0, 255) in float32; NaN -> 0"""
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.asarray(x, np.float32) + np.float32(1.0)) * np.float32(127.5)
        v = np.floor(t + np.float32(0.5))
    return np.clip(np.where(np.isnan(v), np.float32(0.0), v), 0.0, 255.0).astype(np.int64)


def ref_table():
    return np.array([lv / 127.5 - 1.0 for lv in range(256)], np.float64).astype(np.float32)


def ref_units(u):
    """levels -> model units through the table"""
    return ref_table()[u]


def _ycc(u):
    r, g, b = u[..., 0, :, :], u[..., 1, :, :], u[..., 2, :, :]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _rgb(y, cb, cr):
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -3), 0, 255)


def ref_dct_table():
    c = [math.sqrt(0.125)] + [0.5] * 7
    return np.array([[math.floor(c[k] * math.cos((2 * n + 1) * k * math.pi / 16.0) * 8192.0 + 0.5) for n in range(8)]
                     for k in range(8)], np.int64)


ANNEX_K_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
                87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                72, 92, 95, 98, 112, 100, 103, 99]
ANNEX_K_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                  47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32


def ref_quant_tables(quality):
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [np.clip((np.array(b, np.int64) * s + 50) // 100, 1, 255).reshape(8, 8) for b in (ANNEX_K_LUMA, ANNEX_K_CHROMA)]


def _codec(p, Q):
    """an 8-bit plane [..., P, P] (P a multiple of 8) through level shift, DCT, quantisation and back"""
    T = ref_dct_table()
    P = p.shape[-1]
    b = (p - 128).reshape(p.shape[:-2] + (P // 8, 8, P // 8, 8)).swapaxes(-3, -2)          # [..., by, bx, m, n]
    t = (np.einsum("km,...mn->...kn", T, b) + (1 << 9)) >> 10                                # columns: Q3
    c = (np.einsum("...kn,ln->...kl", t, T) + (1 << 12)) >> 13                               # rows: eight times the coefficient
    r = np.sign(c) * ((np.abs(c) + 4 * Q) // (8 * Q) * Q)                                    # round half away, de-quantise
    t = (np.einsum("km,...kl->...ml", T, r) + (1 << 10)) >> 11                               # inverse columns: Q2
    o = (np.einsum("...ml,ln->...mn", t, T) + (1 << 14)) >> 15
    return np.clip(o + 128, 0, 255).swapaxes(-3, -2).reshape(p.shape)


def _upsample(c):
    """[..., H, W] -> [..., 2H, 2W]: triangle filter, edges replicated, bias 8 on even and 7 on odd output columns"""
    pad = [(0, 0)] * (c.ndim - 2)
    cp = np.pad(c, pad + [(1, 1), (0, 0)], mode="edge")
    v = np.stack([3 * c + cp[..., :-2, :], 3 * c + cp[..., 2:, :]], -2).reshape(c.shape[:-2] + (2 * c.shape[-2], c.shape[-1]))
    vp = np.pad(v, pad + [(0, 0), (1, 1)], mode="edge")
    o = np.stack([(3 * v + vp[..., :-2] + 8) >> 4, (3 * v + vp[..., 2:] + 7) >> 4], -1)
    return o.reshape(v.shape[:-1] + (2 * c.shape[-1],))


def ref_jpeg(u, quality, subsampling="420"):
    """levels [..., 3, S, S] -> levels after JPEG at `quality`"""
    u = np.asarray(u, np.int64)
    S = u.shape[-1]
    mcu = 16 if subsampling == "420" else 8
    P = (S + mcu - 1) // mcu * mcu
    up = np.pad(u, [(0, 0)] * (u.ndim - 2) + [(0, P - S), (0, P - S)], mode="edge")
    y, cb, cr = _ycc(up)
    if subsampling == "420":
        cb, cr = [(c[..., 0::2, 0::2] + c[..., 0::2, 1::2] + c[..., 1::2, 0::2] + c[..., 1::2, 1::2] + 2) >> 2 for c in (cb, cr)]
    ql, qc = ref_quant_tables(quality)
    y, cb, cr = _codec(y, ql), _codec(cb, qc), _codec(cr, qc)
    if subsampling == "420":
        cb, cr = _upsample(cb), _upsample(cr)
    return _rgb(y, cb, cr)[..., :S, :S]


def ref_blur_weights(k):
    r, sigma = k // 2, 0.3 * ((k - 1) / 2.0 - 1.0) + 0.8
    g = [math.exp(-((i - r) ** 2) / (2.0 * sigma * sigma)) for i in range(k)]
    w = [math.floor(v / sum(g) * 16384.0 + 0.5) for v in g]
    w[r] += 16384 - sum(w)
    return np.array(w, np.int64)


def ref_blur(u, k):
    u = np.asarray(u, np.int64)
    w, r, S = ref_blur_weights(k), k // 2, u.shape[-1]
    assert S >= r + 1
    pad = [(0, 0)] * (u.ndim - 2)
    p = np.pad(u, pad + [(0, 0), (r, r)], mode="reflect")
    h = (sum(w[j] * p[..., :, j:j + S] for j in range(k)) + (1 << 13)) >> 14
    p = np.pad(h, pad + [(r, r), (0, 0)], mode="reflect")
    return (sum(w[j] * p[..., j:j + S, :] for j in range(k)) + (1 << 13)) >> 14


def _about_128(u, f8):
    return np.clip(128 + (((u - 128) * f8 + 128) >> 8), 0, 255)


def ref_point(u, kind, f8=0, s=0.0, z=None):
    u = np.asarray(u, np.int64)
    if kind == "contrast":
        return _about_128(u, f8)
    if kind == "saturation":
        y, cb, cr = _ycc(u)
        return _rgb(y, _about_128(cb, f8), _about_128(cr, f8))
    with np.errstate(invalid="ignore", over="ignore"):
        v = u.astype(np.float32) + np.float32(s) * np.asarray(z, np.float32)
        v = np.floor(v + np.float32(0.5))
    return np.clip(np.where(np.isnan(v), np.float32(0.0), v), 0.0, 255.0).astype(np.int64)


def ref_pixelate(u, f):
    u = np.asarray(u, np.int64)
    S = u.shape[-1]
    idx = np.arange(0, S, f)
    cells = lambda a: np.add.reduceat(np.add.reduceat(a, idx, axis=-2), idx, axis=-1)
    s, cnt = cells(u), cells(np.ones((S, S), np.int64))
    m = (s + cnt // 2) // cnt
    return np.repeat(np.repeat(m, f, axis=-2), f, axis=-1)[..., :S, :S]


def ref_blocks(u, pos):
    """u [N, 3, S, S]; pos [N, count, 2] (row, column)"""
    o = np.array(u, np.int64)
    S = o.shape[-1]
    for n in range(o.shape[0]):
        for yy, xx in np.asarray(pos[n]).reshape(-1, 2):
            o[n, :, max(yy, 0):max(min(yy + 8, S), 0), max(xx, 0):max(min(xx + 8, S), 0)] = 128
    return o


def ref_apply(u, stage, subsampling="420", extra=None):
    """one resolved stage (name, parameter) of corrupt.resolve on levels"""
    kind, p = stage
    if kind == "jpeg":
        return ref_jpeg(u, p, subsampling)
    if kind == "gaussian_blur":
        return ref_blur(u, p)
    if kind == "gaussian_noise":
        return ref_point(u, kind, s=np.float32(255.0 * math.sqrt(p)), z=extra)
    if kind == "pixelate":
        return ref_pixelate(u, p)
    if kind == "block":
        return ref_blocks(u, extra)
    return ref_point(u, kind, f8=math.floor(256.0 * p + 0.5))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def pil_images():
    """two seeded 128 x 128 uint8 images [3, 128, 128]: three sinusoid planes plus N(0, 8) noise; half that base plus 64 plus
    N(0, 40) noise"""
    rng = np.random.default_rng(20)
    yy, xx = np.meshgrid(np.arange(128.0), np.arange(128.0), indexing="ij")
    base = np.stack([128.0 + 100.0 * np.sin(2.0 * np.pi * (fx * xx + fy * yy) / 128.0 + ph)
                     for fx, fy, ph in ((1.0, 2.0, 0.0), (3.0, 1.0, 1.0), (2.0, 5.0, 2.0))])
    a = base + rng.normal(0.0, 8.0, base.shape)
    b = base / 2.0 + 64.0 + rng.normal(0.0, 40.0, base.shape)
    return [np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8) for v in (a, b)]


# ---- tables ------------------------------------------------------------------------------------------------------------------------
def test_level_table_round_trips():
    t = ref_table()
    assert np.array_equal(ref_quantise(t), np.arange(256))
    assert np.array_equal(np.array(CR.level_table(), np.float64).astype(np.float32), t)
    assert t[0] == -1.0 and t[255] == 1.0
    # a NaN is level 0, +-inf and anything outside [-1, 1] clamp
    assert ref_quantise(np.array([np.nan, -np.inf, np.inf, -3.0, 3.0, 0.0], np.float32)).tolist() == [0, 0, 255, 0, 255, 128]


def test_quality_rule():
    assert all(np.array_equal(t, np.ones((8, 8))) for t in ref_quant_tables(100))
    assert np.array_equal(ref_quant_tables(50)[0].ravel(), ANNEX_K_LUMA) and np.array_equal(ref_quant_tables(50)[1].ravel(), ANNEX_K_CHROMA)
    assert tuple(CR.JPEG_LUMA) == tuple(ANNEX_K_LUMA) and tuple(CR.JPEG_CHROMA) == tuple(ANNEX_K_CHROMA)
    for q in range(1, 101):
        got, want = CR.jpeg_tables(q), ref_quant_tables(q)
        assert [list(t) for t in got] == [w.ravel().tolist() for w in want]
        assert all(1 <= v <= 255 for t in got for v in t)


_ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
           42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


@pytest.mark.parametrize("quality", CR.LEVELS["jpeg"])
def test_quantisation_tables_are_the_ones_pil_writes(quality):
    Image = pytest.importorskip("PIL.Image")
    import PIL
    buf = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(buf, format="JPEG", quality=quality)
    buf.seek(0)
    q = Image.open(buf).quantization
    natural = tuple(int(v) for v in PIL.__version__.split(".")[:2]) >= (8, 3)     # earlier versions hand the file's zigzag order out
    for got, want in zip((q[0], q[1]), CR.jpeg_tables(quality)):
        got = list(got)
        if not natural:
            nat = [0] * 64
            for i, z in enumerate(_ZIGZAG):
                nat[z] = got[i]
            got = nat
        assert got == list(want)


def test_blur_weights():
    for k in range(1, CR.BLUR_MAX_K + 1, 2):
        w = ref_blur_weights(k)
        assert tuple(w.tolist()) == CR.blur_weights(k)
        assert w.sum() == 1 << 14 and np.array_equal(w, w[::-1]) and (w >= 0).all() and w[k // 2] == w.max()
    assert CR.blur_sigma(7) == pytest.approx(1.4) and CR.blur_sigma(21) == pytest.approx(3.5)


def test_dct_table_is_orthogonal():
    T = ref_dct_table()
    assert tuple(map(tuple, T.tolist())) == CR.dct_table()
    t = T.astype(np.float64) / 8192.0
    assert np.abs(t @ t.T - np.eye(8)).max() <= 2.0 ** -11
    assert np.abs(T).max() == 4017 and np.abs(T).sum(1).max() <= 8 * 4017        # the kernel's no-overflow bounds rest on these


def test_int32_is_enough_for_any_8_bit_block():
    """the bounds written in csrc/corrupt.hip, evaluated: worst-case row sums through the four passes stay below 2^31"""
    row = 8 * 4017
    t1 = (row * 128 + 512) >> 10
    c = (row * t1 + 4096) >> 13
    r = (c + 4 * 255) // 8
    t2 = (row * r + 1024) >> 11
    assert max(row * 128, row * t1, row * r, row * t2) + (1 << 14) < 2 ** 31 and max(t1, c, r, t2) < 2 ** 23


# ---- exact cases -------------------------------------------------------------------------------------------------------------------
def _const(level, S=24):
    return np.full((3, S, S), level, np.int64)


@pytest.mark.parametrize("subsampling", CR.SUBSAMPLINGS)
@pytest.mark.parametrize("quality", [100, 90, 70, 50, 30, 10, 1])
def test_constant_image_survives_jpeg(quality, subsampling):
    ql, qc = ref_quant_tables(quality)
    dc_l, dc_c = int(ql[0, 0]), int(qc[0, 0])
    for lv in (128, 128 + dc_l, 128 - dc_l):                       # constants every quality represents: within the colour rounding
        if 0 <= lv <= 255:
            assert np.abs(ref_jpeg(_const(lv), quality, subsampling) - lv).max() <= 1
    rgb = np.array([200, 60, 120], np.int64).reshape(3, 1, 1) + np.zeros((3, 24, 24), np.int64)
    for u in (_const(7), _const(251), rgb):                        # any constant: half a DC step of luma and chroma besides
        o = ref_jpeg(u, quality, subsampling)
        assert (o == o[:, :1, :1]).all()                           # still constant
        bound = 1 + (dc_l / 16.0 + 1.0) + 1.772 * (dc_c / 16.0 + 1.0)
        assert np.abs(o - u).max() <= bound


def test_identities():
    rng = np.random.default_rng(3)
    u = rng.integers(0, 256, (2, 3, 21, 21))
    for lv in (0, 77, 128, 255):
        c = _const(lv, 21)
        for k in (1, 7, 21):
            assert np.array_equal(ref_blur(c, k), c)
        for f in (1, 2, 6, 21, 25):
            assert np.array_equal(ref_pixelate(c, f), c)
        assert np.array_equal(ref_point(c, "saturation", f8=256), c)
    assert np.array_equal(ref_point(u, "contrast", f8=256), u)
    assert np.array_equal(ref_pixelate(u, 1), u)
    assert np.array_equal(ref_blur(u, 1), u)
    assert np.array_equal(ref_blocks(u, np.zeros((2, 0, 2), np.int64)), u)
    assert np.array_equal(ref_point(u, "gaussian_noise", s=0.0, z=np.ones(u.shape, np.float32)), u)
    # grey stays grey under saturation 0, and saturation 0 makes every pixel grey to within the colour rounding
    g = ref_point(u, "saturation", f8=0)
    assert np.abs(g - g[:, :1]).max() <= 1


def test_pixelate_edge_cells_use_their_own_count():
    u = np.arange(25, dtype=np.int64).reshape(1, 5, 5) * 10
    o = ref_pixelate(u, 3)
    assert o[0, 0, 0] == (u[0, :3, :3].sum() + 4) // 9 and o[0, 4, 4] == (u[0, 3:, 3:].sum() + 2) // 4
    assert o[0, 0, 4] == (u[0, :3, 3:].sum() + 3) // 6


@pytest.mark.parametrize("subsampling", CR.SUBSAMPLINGS)
@pytest.mark.parametrize("S", [8, 20, 44])
def test_jpeg_pads_by_replication(S, subsampling):
    rng = np.random.default_rng(S)
    u = rng.integers(0, 256, (3, S, S))
    mcu = 16 if subsampling == "420" else 8
    P = (S + mcu - 1) // mcu * mcu
    padded = np.pad(u, [(0, 0), (0, P - S), (0, P - S)], mode="edge")
    for q in (90, 10):
        assert np.array_equal(ref_jpeg(u, q, subsampling), ref_jpeg(padded, q, subsampling)[:, :S, :S])


def test_blocks_are_clipped():
    u = np.zeros((1, 3, 20, 20), np.int64)
    o = ref_blocks(u, np.array([[[-7, -7], [-8, 3], [15, 15], [19, -3], [6, 6], [40, 40]]]))
    want = np.zeros((20, 20), np.int64)
    want[0, 0] = want[15:, 15:] = want[19, :5] = want[6:14, 6:14] = 128
    assert np.array_equal(o[0, 0], want) and np.array_equal(o[0, 1], want)


# ---- against PIL -----------------------------------------------------------------------------------------------------------------
PIL_BAR = 0.25


@pytest.mark.parametrize("subsampling", CR.SUBSAMPLINGS)
@pytest.mark.parametrize("quality", [90, 50, 10])
@pytest.mark.parametrize("which", [0, 1])
def test_jpeg_against_pil(which, quality, subsampling):
    """the integer restatement is a JPEG: its mean absolute difference from PIL's save-and-reload is at most 0.25 of PIL's own
    mean absolute difference from the clean image"""
    Image = pytest.importorskip("PIL.Image")
    img = pil_images()[which]
    buf = io.BytesIO()
    Image.fromarray(img.transpose(1, 2, 0)).save(buf, format="JPEG", quality=quality, subsampling={"420": 2, "444": 0}[subsampling])
    buf.seek(0)
    pil = np.asarray(Image.open(buf).convert("RGB")).transpose(2, 0, 1).astype(np.int64)
    ours = ref_jpeg(img.astype(np.int64), quality, subsampling)
    ratio = np.abs(ours - pil).mean() / np.abs(pil - img.astype(np.int64)).mean()
    print(f"  image {which} quality {quality} {subsampling}: ratio {ratio:.4f}")
    assert ratio <= PIL_BAR


# ---- monotone --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", CR.CORRUPTIONS)
def test_severity_is_monotone(kind):
    u = pil_images()[0].astype(np.int64)[None]
    rng = np.random.default_rng(9)
    z = rng.standard_normal(u.shape).astype(np.float32)
    pos = rng.integers(-7, 128, (1, 80, 2))
    change = []
    for level in range(1, 6):
        stage, = CR.resolve(kind, level)
        extra = z if kind == "gaussian_noise" else (pos[:, :stage[1]] if kind == "block" else None)
        change.append(float(np.abs(ref_apply(u, stage, extra=extra) - u).mean()))
    print(f"  {kind}: {[round(c, 3) for c in change]}")
    assert all(a < b for a, b in zip(change, change[1:])), change


# ---- resolve and the entry points' refusals ------------------------------------------------------------------------------------------
def test_resolve():
    assert CR.CORRUPTIONS == ("jpeg", "gaussian_blur", "gaussian_noise", "pixelate", "contrast", "saturation", "block")
    assert CR.LEVELS["jpeg"] == (90, 70, 50, 30, 10) and CR.LEVELS["gaussian_blur"] == (7, 9, 13, 17, 21)
    assert CR.LEVELS["gaussian_noise"] == (0.001, 0.002, 0.005, 0.01, 0.05) and CR.LEVELS["pixelate"] == (2, 3, 4, 5, 6)
    assert CR.LEVELS["contrast"] == (0.85, 0.725, 0.6, 0.475, 0.35) and CR.LEVELS["saturation"] == (0.4, 0.3, 0.2, 0.1, 0.0)
    assert CR.LEVELS["block"] == (16, 32, 48, 64, 80)
    assert CR.resolve("jpeg", 3) == (("jpeg", 50),)
    assert CR.resolve("jpeg", 3, param=35) == (("jpeg", 35),) and CR.resolve("contrast", param=1) == (("contrast", 1.0),)
    assert CR.resolve([("gaussian_blur", 3), ("jpeg", 4)]) == (("gaussian_blur", 13), ("jpeg", 30))
    assert CR.resolve([("pixelate", {"param": 8}), ["block", {"level": 1}]]) == (("pixelate", 8), ("block", 16))


@pytest.mark.parametrize("args,kw", [
    (("jpg", 3), {}), ((None, 3), {}), (("jpeg", 0), {}), (("jpeg", 6), {}), (("jpeg", 2.0), {}), (("jpeg", True), {}), (("jpeg",), {}),
    (("jpeg",), {"param": 0}), (("jpeg",), {"param": 101}), (("jpeg",), {"param": 50.0}), (("gaussian_blur",), {"param": 8}),
    (("gaussian_blur",), {"param": 33}), (("gaussian_noise",), {"param": -0.1}), (("gaussian_noise",), {"param": float("nan")}),
    (("pixelate",), {"param": 0}), (("pixelate",), {"param": 257}), (("contrast",), {"param": -1.0}), (("block",), {"param": -1}),
    (("block",), {"param": 1025}), (([],), {}), (([("jpeg", 3, 4)],), {}), (([("jpeg", {})],), {}),
    (([("jpeg", {"level": 3, "param": 50})],), {}), (([("jpeg", {"quality": 50})],), {}), (([("jpeg", None)],), {}), (([("jpeg", 9)],), {}),
    ((["jpeg"],), {}),
])
def test_resolve_refuses(args, kw):
    with pytest.raises(ValueError):
        CR.resolve(*args, **kw)


def test_entry_points_refuse_invalid_arguments_without_a_device():
    import ctypes as C
    from unidefense_amd import lib
    L = lib.load()
    a, b, t, tab = (C.c_void_p(v) for v in (4096, 8192, 12288, 16384))       # never dereferenced: validation comes first
    nan = float("nan")
    bad = [
        ("ud_corrupt_jpeg", (None, b, t, tab, 1, 16, 50, 0, None)), ("ud_corrupt_jpeg", (a, None, t, tab, 1, 16, 50, 0, None)),
        ("ud_corrupt_jpeg", (a, b, None, tab, 1, 16, 50, 0, None)), ("ud_corrupt_jpeg", (a, b, t, None, 1, 16, 50, 0, None)),
        ("ud_corrupt_jpeg", (a, a, t, tab, 1, 16, 50, 0, None)),
        ("ud_corrupt_jpeg", (a, b, t, tab, 0, 16, 50, 0, None)), ("ud_corrupt_jpeg", (a, b, t, tab, 65536, 16, 50, 0, None)),
        ("ud_corrupt_jpeg", (a, b, t, tab, 1, 0, 50, 0, None)), ("ud_corrupt_jpeg", (a, b, t, tab, 1, 32769, 50, 0, None)),
        ("ud_corrupt_jpeg", (a, b, t, tab, 1, 16, 0, 0, None)), ("ud_corrupt_jpeg", (a, b, t, tab, 1, 16, 101, 0, None)),
        ("ud_corrupt_jpeg", (a, b, t, tab, 1, 16, 50, 2, None)),
        ("ud_corrupt_blur", (None, b, t, tab, 1, 16, 7, None)), ("ud_corrupt_blur", (a, b, t, None, 1, 16, 7, None)),
        ("ud_corrupt_blur", (a, b, t, tab, 0, 16, 7, None)), ("ud_corrupt_blur", (a, b, t, tab, 1, 32769, 7, None)),
        ("ud_corrupt_blur", (a, b, t, tab, 1, 16, 8, None)), ("ud_corrupt_blur", (a, b, t, tab, 1, 16, 0, None)),
        ("ud_corrupt_blur", (a, b, t, tab, 1, 64, 33, None)), ("ud_corrupt_blur", (a, b, t, tab, 1, 10, 21, None)),
        ("ud_corrupt_point", (None, b, t, None, 1, 16, 0, 256, 0.0, None)), ("ud_corrupt_point", (a, b, t, None, 70000, 16, 0, 256, 0.0, None)),
        ("ud_corrupt_point", (a, b, t, None, 1, 0, 0, 256, 0.0, None)), ("ud_corrupt_point", (a, b, t, None, 1, 16, 3, 256, 0.0, None)),
        ("ud_corrupt_point", (a, b, t, None, 1, 16, 0, -1, 0.0, None)), ("ud_corrupt_point", (a, b, t, None, 1, 16, 1, 65537, 0.0, None)),
        ("ud_corrupt_point", (a, b, t, None, 1, 16, 2, 0, 1.0, None)), ("ud_corrupt_point", (a, b, t, tab, 1, 16, 2, 0, nan, None)),
        ("ud_corrupt_point", (a, b, t, tab, 1, 16, 2, 0, -1.0, None)),
        ("ud_corrupt_pixelate", (None, b, t, 1, 16, 2, None)), ("ud_corrupt_pixelate", (a, b, t, 1, 16, 0, None)),
        ("ud_corrupt_pixelate", (a, b, t, 1, 16, 257, None)), ("ud_corrupt_pixelate", (a, b, t, 0, 16, 2, None)),
        ("ud_corrupt_pixelate", (a, b, t, 1, 40000, 2, None)),
        ("ud_corrupt_blocks", (None, b, t, tab, 1, 16, 4, None)), ("ud_corrupt_blocks", (a, b, t, None, 1, 16, 4, None)),
        ("ud_corrupt_blocks", (a, b, t, tab, 1, 16, -1, None)), ("ud_corrupt_blocks", (a, b, t, tab, 1, 16, 1025, None)),
        ("ud_corrupt_blocks", (a, b, t, tab, 65536, 16, 4, None)), ("ud_corrupt_blocks", (a, b, t, tab, 1, 0, 4, None)),
    ]
    for name, args in bad:
        assert getattr(L, name)(*args) == -1000, (name, args)
    for name in ("ud_corrupt_jpeg", "ud_corrupt_blur", "ud_corrupt_point", "ud_corrupt_pixelate", "ud_corrupt_blocks"):
        assert name in lib.EXPORTED


def test_host_side_refusals_need_no_device():
    import torch
    from unidefense_amd.model import load_model
    m = load_model("UDR18")(num_classes=2).eval()
    with pytest.raises(ValueError, match="cuda"):
        CR.corrupt(torch.zeros(1, 3, 16, 16), "jpeg")
    with pytest.raises(ValueError, match="subsampling"):
        CR.corrupt(torch.zeros(1, 3, 16, 16), "jpeg", subsampling="422")
    for kw, match in (({"kind": "jpg"}, "corruption"), ({"kind": "jpeg", "level": 6}, "level"),
                      ({"kind": "jpeg", "level": None}, "level"), ({"kind": [("jpeg", {"level": 1, "param": 2})]}, "exactly one"),
                      ({"kind": "jpeg", "subsampling": "411"}, "subsampling"), ({"kind": "gaussian_blur", "level": 5, "size": 10}, "blur"),
                      ({"kind": "jpeg", "precision": "fp16"}, "fp16"), ({"kind": "jpeg"}, "cuda")):
        kw = dict(kw)
        kind, size = kw.pop("kind"), kw.pop("size", 64)
        for make in (lambda: CR.CorruptionRunner(m, 2, size, kind, **kw), lambda: CR.corruption_runner(m, 2, size, kind, **kw),
                     lambda: m.corruption_runner(2, size, kind, **kw)):
            with pytest.raises(ValueError, match=match):
                make()
    m.train()
    with pytest.raises(ValueError, match="eval"):
        m.corruption_runner(2, 64, "jpeg")
    assert not m.__dict__.get("_ud_corruption_runners")
