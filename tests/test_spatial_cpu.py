"""CPU: the affine warp's definition (include/unidefense_hip.h: ud_warp_affine) restated in numpy — ref_warp, which the GPU
tests compare csrc/warp.hip against bit for bit — its exactness properties, its agreement with grid_sample, the host tables
(affine_q16, spatial_candidates) and every refusal that needs no device."""
import ctypes
import math

import numpy as np
import pytest
import torch

from unidefense_amd import spatial as SP

SIZES = (8, 20, 44, 128)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def ref_index(i, S, border):
    """(index, inside) of the int64 coordinates i under the border rule; outside only under "fill" """
    i = np.asarray(i, np.int64)
    if border == "reflect":
        if S == 1:
            return np.zeros_like(i), np.ones(i.shape, bool)
        p = 2 * (S - 1)
        j = np.mod(i, p)                                   # numpy's mod is the mathematical one
        return np.where(j >= S, p - j, j), np.ones(i.shape, bool)
    if border == "edge":
        return np.clip(i, 0, S - 1), np.ones(i.shape, bool)
    assert border == "fill"
    return np.clip(i, 0, S - 1), (i >= 0) & (i <= S - 1)


def ref_warp(levels, mats, border="reflect"):
    """levels int64 [N, 3, S, S] warped by mats [N, 6] (one row per sample; [6]: the same for all), in int64 throughout"""
    u = np.asarray(levels, np.int64)
    N, _, S, _ = u.shape
    mats = np.broadcast_to(np.asarray(mats, np.int64).reshape(-1, 6), (N, 6)) if np.asarray(mats).size == 6 else np.asarray(mats, np.int64)
    assert mats.shape == (N, 6)
    X = (2 * np.arange(S, dtype=np.int64) + 1 - S)[None, :]           # by column
    Y = (2 * np.arange(S, dtype=np.int64) + 1 - S)[:, None]           # by row
    out = np.empty_like(u)
    centre = np.int64(S - 1) << 16
    for n in range(N):
        m00, m01, o0, m10, m11, o1 = (np.int64(v) for v in mats[n])
        px = (m00 * X + m01 * Y + o0 + centre) >> 1
        py = (m10 * X + m11 * Y + o1 + centre) >> 1
        x0, fx, y0, fy = px >> 16, (px >> 8) & 255, py >> 16, (py >> 8) & 255
        taps = []
        for dy in (0, 1):
            for dx in (0, 1):
                sy, iny = ref_index(y0 + dy, S, border)
                sx, inx = ref_index(x0 + dx, S, border)
                taps.append(np.where((iny & inx)[None], u[n][:, sy, sx], 128))
        u00, u01, u10, u11 = taps
        out[n] = ((256 - fx) * (256 - fy) * u00 + fx * (256 - fy) * u01 + (256 - fx) * fy * u10 + fx * fy * u11 + 32768) >> 16
    return out


def _levels(S, N=2, seed=0):
    return np.random.default_rng(100 * S + seed).integers(0, 256, (N, 3, S, S)).astype(np.int64)


# ---- affine_q16 ----------------------------------------------------------------------------------------------------------------------
def test_affine_q16_values():
    assert SP.affine_q16() == (65536, 0, 0, 0, 65536, 0)
    assert SP.affine_q16(angle=90) == (0, 65536, 0, -65536, 0, 0)
    assert SP.affine_q16(angle=180) == (-65536, 0, 0, 0, -65536, 0)
    assert SP.affine_q16(angle=270) == (0, -65536, 0, 65536, 0, 0)
    assert SP.affine_q16(flip=True) == (-65536, 0, 0, 0, 65536, 0)
    assert SP.affine_q16(shift=(3, -2)) == (65536, 0, -6 * 65536, 0, 65536, 4 * 65536)
    assert SP.affine_q16(scale=0.5) == (131072, 0, 0, 0, 131072, 0)
    # by hand: A^-1 = 1.25 [[cos 30, sin 30], [-sin 30, cos 30]] = [[1.0825317547, 0.625], [-0.625, 1.0825317547]];
    # -A^-1 (2.5, -1.25) = (-1.9250793868, 2.9156646934); m = round(. 65536), o = round(2 . 65536)
    assert SP.affine_q16(30.0, 0.8, (2.5, -1.25)) == (70945, 40960, -252324, -40960, 70945, 382162)
    # the flip acts on the source's x before the rotation: the first column of A changes sign, so the first ROW of A^-1 does
    a, b = SP.affine_q16(30.0, 0.8, (0, 0)), SP.affine_q16(30.0, 0.8, (0, 0), flip=True)
    assert b == (-a[0], -a[1], 0, a[3], a[4], 0)


@pytest.mark.parametrize("kw", [{"scale": 0.0}, {"scale": -1.0}, {"scale": float("nan")}, {"angle": float("inf")},
                                {"shift": (float("nan"), 0.0)}, {"scale": 1e-6}, {"shift": (1e6, 0.0)}])
def test_affine_q16_refuses(kw):
    with pytest.raises(ValueError):
        SP.affine_q16(**kw)


# ---- exactness -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", SIZES)
def test_exactness_properties(S):
    u = _levels(S)
    for border in SP.BORDERS:
        assert np.array_equal(ref_warp(u, SP.affine_q16(), border), u)
        assert np.array_equal(ref_warp(u, SP.affine_q16(flip=True), border), u[..., ::-1])
        for k, angle in ((-1, 90), (-2, 180), (-3, 270)):
            assert np.array_equal(ref_warp(u, SP.affine_q16(angle=angle), border), np.rot90(u, k, (2, 3))), (border, angle)
        # out(r, c) = in(r + 2, c - 3) wherever the source lies inside
        got = ref_warp(u, SP.affine_q16(shift=(3, -2)), border)
        assert np.array_equal(got[:, :, :S - 2, 3:], u[:, :, 2:, :S - 3])
    # a different map per sample
    got = ref_warp(u, [SP.affine_q16(flip=True), SP.affine_q16(angle=180)])
    assert np.array_equal(got[0], u[0][..., ::-1]) and np.array_equal(got[1], u[1][:, ::-1, ::-1])


@pytest.mark.parametrize("S", SIZES)
def test_far_shift_in_each_border_mode(S):
    u = _levels(S, seed=1)
    m = SP.affine_q16(shift=(3 * S + 0.5, 3 * S + 0.5))              # source = output - 3 S - 0.5: taps at c - 3 S - 1 and c - 3 S
    assert np.array_equal(ref_warp(u, m, "fill"), np.full_like(u, 128))
    assert np.array_equal(ref_warp(u, m, "edge"), np.broadcast_to(u[:, :, :1, :1], u.shape))
    # along x only: every output column blends the replicated first column with itself
    mx = SP.affine_q16(shift=(3 * S + 0.5, 0))
    assert np.array_equal(ref_warp(u, mx, "edge"), np.broadcast_to(u[:, :, :, :1], u.shape))
    # reflect-101 against an explicit pad, built wide enough in steps of at most S - 1 (np.pad's own reflect limit is met by
    # padding repeatedly: reflecting a reflect-101 extension about its new edge continues the same periodic pattern)
    pad = 3 * S + 2
    wide, have = u, 0
    while have < pad:
        step = min(wide.shape[-1] - 1, pad - have)
        wide = np.pad(wide, [(0, 0), (0, 0), (step, step), (step, step)], mode="reflect")
        have += step
    # tap (r + dr - 3 S - 1, c + dc - 3 S - 1), dr, dc in {0, 1}, each with weight 1/4: (a + b + c + d + 2) >> 2 in the
    # definition's Q16 form
    base = pad - 3 * S - 1
    t = [wide[:, :, base + dr:base + dr + S, base + dc:base + dc + S] for dr in (0, 1) for dc in (0, 1)]
    want = (16384 * (t[0] + t[1] + t[2] + t[3]) + 32768) >> 16
    assert np.array_equal(ref_warp(u, m, "reflect"), want)


def test_size_one_and_index_rule():
    u = np.array([7, 200, 31], np.int64).reshape(1, 3, 1, 1)
    assert np.array_equal(ref_warp(u, SP.affine_q16(17.0, 0.7, (5.5, -9.25)), "reflect"), u)
    assert np.array_equal(ref_warp(u, SP.affine_q16(17.0, 0.7, (5.5, -9.25)), "edge"), u)
    idx, _ = ref_index(np.arange(-9, 10), 4, "reflect")
    assert idx.tolist() == [3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3]
    idx, inside = ref_index(np.arange(-2, 6), 4, "fill")
    assert inside.tolist() == [False, False, True, True, True, True, False, False]


GRID_SAMPLE_TRANSFORMS = [dict(angle=5.0), dict(angle=-30.0, scale=0.8, flip=True), dict(angle=45.0, scale=1.25), dict(scale=0.5),
                          dict(shift=(0.5, 0.25)), dict(angle=17.0, scale=0.9, shift=(4.5, -3.25))]


def _grid_sample(u, angle=0.0, scale=1.0, shift=(0.0, 0.0), flip=False):
    """float64 grid_sample(bilinear, align_corners=False, padding_mode="border") of the same map: theta is A^-1 in the
    normalised coordinates of affine_grid (pixel = normalised S / 2 about the centre)"""
    S = u.shape[-1]
    c, s = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    f = -1.0 if flip else 1.0
    inv = np.array([[f * c, f * s], [-s, c]]) / scale
    t = -inv @ np.array(shift, np.float64) * 2.0 / S
    theta = torch.tensor(np.concatenate([inv, t[:, None]], 1), dtype=torch.float64).unsqueeze(0).repeat(u.shape[0], 1, 1)
    x = torch.from_numpy(u.astype(np.float64))
    grid = torch.nn.functional.affine_grid(theta, list(x.shape), align_corners=False)
    return torch.nn.functional.grid_sample(x, grid, mode="bilinear", padding_mode="border", align_corners=False).numpy()


def test_agrees_with_grid_sample():
    """Border "edge" against float64 grid_sample over the six transforms and S = 8, 20, 44, 128.  Derived bound for uniform
    random levels: 0.5 (final rounding) + 2 * 255 / 256 (an 8-bit fraction truncated on each axis against a level difference
    of at most 255) + a Q16 coordinate term below 0.1 = about 2.6; bars: 3 levels on noise, 0.75 on a ramp of slope one level
    per pixel (0.5 + 2 / 256 + the coordinate term).  Measured when the definition was written: 2.15 on noise, 0.504 on the
    ramp; with this test's seeds and ramp: 1.74 and 0.5002 (printed below)."""
    worst = {"noise": 0.0, "ramp": 0.0}
    for S in SIZES:
        noise = _levels(S, seed=2)
        ramp = np.broadcast_to(np.arange(S, dtype=np.int64) + 20, (1, 3, S, S)).copy()      # one level per pixel along the columns
        ramp[:, 1] = ramp[:, 1].transpose(0, 2, 1)                     # one channel ramps down the rows
        for kw in GRID_SAMPLE_TRANSFORMS:
            m = SP.affine_q16(**kw)
            for name, u in (("noise", noise), ("ramp", ramp)):
                d = np.abs(ref_warp(u, m, "edge") - _grid_sample(u, **kw)).max()
                worst[name] = max(worst[name], float(d))
    print("largest difference from grid_sample, levels:", worst)
    assert worst["noise"] <= 3.0 and worst["ramp"] <= 0.75, worst


# ---- candidates ----------------------------------------------------------------------------------------------------------------------
def test_grid_candidates():
    t = SP.spatial_candidates(128, 10.0, 0.05, (0.9, 1.1), False, "grid", (3, 2, 2), batch=3)
    assert t.dtype == torch.float64 and tuple(t.shape) == (1 + 3 * 2 * 2 * 2, 3, 5)
    assert t[0].tolist() == [[0.0, 0.0, 0.0, 1.0, 0.0]] * 3
    assert torch.equal(t[:, 0], t[:, 1]) and torch.equal(t[:, 0], t[:, 2])
    want = [[a, dx, dy, z, 0.0] for a in (-10.0, 0.0, 10.0) for dx in (-6.4, 6.4) for dy in (-6.4, 6.4) for z in (0.9, 1.1)]
    assert np.allclose(t[1:, 0].numpy(), np.array(want), rtol=0, atol=1e-12)
    assert t[1:, 0, 0].tolist()[::8] == [-10.0, 0.0, 10.0] and t[-1, 0].tolist() == [10.0, 0.05 * 128, 0.05 * 128, 1.1, 0.0]
    # flip doubles the grid, the mirrored half second
    tf = SP.spatial_candidates(128, 10.0, 0.05, (0.9, 1.1), True, "grid", (3, 2, 2))
    assert tuple(tf.shape) == (1 + 2 * 24, 1, 5)
    assert torch.equal(tf[1:25, 0, :4], t[1:, 0, :4]) and torch.equal(tf[25:, 0, :4], t[1:, 0, :4])
    assert tf[1:25, 0, 4].eq(0).all() and tf[25:, 0, 4].eq(1).all()
    # counts of 1 give the neutral values; the default grid
    assert SP.spatial_candidates(64, grid=(1, 1, 1)).reshape(-1, 5).tolist() == [[0.0, 0.0, 0.0, 1.0, 0.0]] * 2
    t1 = SP.spatial_candidates(64, grid=(1, 3, 1))
    assert tuple(t1.shape) == (10, 1, 5) and t1[:, 0, 0].eq(0).all() and t1[:, 0, 3].eq(1).all()
    assert t1[1:, 0, 1].tolist() == [-3.2, -3.2, -3.2, 0.0, 0.0, 0.0, 3.2, 3.2, 3.2]
    assert t1[1:, 0, 2].tolist() == [-3.2, 0.0, 3.2] * 3
    assert SP.spatial_candidates(380).shape[0] == 1 + 7 * 5 * 5 * 3
    assert SP.spatial_candidates(128, grid=(3, 2, 1)).shape[0] == 13
    # a zero range is a grid of equal candidates, not an error
    assert SP.spatial_candidates(64, max_angle=0.0, max_shift=0.0, scales=(1.0, 1.0), grid=(3, 2, 2))[:, 0].unique(dim=0).shape[0] == 1


def test_random_candidates():
    g = lambda seed: torch.Generator().manual_seed(seed)
    kw = dict(max_angle=15.0, max_shift=0.1, scales=(0.8, 1.2), flip=True, search="random", k=50, batch=4)
    a, b, c = SP.spatial_candidates(100, generator=g(3), **kw), SP.spatial_candidates(100, generator=g(3), **kw), \
        SP.spatial_candidates(100, generator=g(4), **kw)
    assert a.dtype == torch.float64 and tuple(a.shape) == (51, 4, 5)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert a[0].tolist() == [[0.0, 0.0, 0.0, 1.0, 0.0]] * 4
    d = a[1:]
    assert d[..., 0].abs().max() <= 15.0 and d[..., 1:3].abs().max() <= 10.0 and d[..., 3].min() >= 0.8 and d[..., 3].max() <= 1.2
    assert set(d[..., 4].unique().tolist()) == {0.0, 1.0}
    assert not torch.equal(d[:, 0], d[:, 1])                         # every sample has draws of its own
    # the documented order of the draws
    gen = g(3)
    u = [torch.rand(50, 4, generator=gen, dtype=torch.float64) for _ in range(4)]
    f = torch.randint(0, 2, (50, 4), generator=gen).double()
    assert torch.equal(d[..., 0], -15.0 + 30.0 * u[0]) and torch.equal(d[..., 2], -10.0 + 20.0 * u[2])
    assert torch.equal(d[..., 3], 0.8 + (1.2 - 0.8) * u[3]) and torch.equal(d[..., 4], f)
    # without flip no flip is drawn, and the default generator is torch's CPU one
    torch.manual_seed(9)
    n1 = SP.spatial_candidates(100, search="random", k=5)
    torch.manual_seed(9)
    assert torch.equal(n1, SP.spatial_candidates(100, search="random", k=5)) and n1[..., 4].eq(0).all()


def test_candidates_q16_is_affine_q16_row_by_row():
    t = SP.spatial_candidates(64, search="random", k=3, batch=2, flip=True, generator=torch.Generator().manual_seed(1))
    q = SP.candidates_q16(t)
    assert q.dtype == torch.int32 and tuple(q.shape) == (8, 6)
    for k in range(4):
        for n in range(2):
            an, dx, dy, z, f = t[k, n].tolist()
            assert tuple(q[k * 2 + n].tolist()) == SP.affine_q16(an, z, (dx, dy), f != 0.0)
    assert q[:2].tolist() == [[65536, 0, 0, 0, 65536, 0]] * 2


BAD = [({"search": "sobol"}, "search"), ({"border": "wrap"}, "border"), ({"objective": "hinge"}, "objective"),
       ({"precision": "bf16"}, "precision"), ({"precision": "fp16"}, "fp16"), ({"max_angle": -1.0}, "max_angle"),
       ({"max_shift": -0.1}, "max_shift"), ({"max_angle": float("nan")}, "max_angle"), ({"scales": (0.0, 1.0)}, "scales"),
       ({"scales": (1.1, 0.9)}, "scales"), ({"scales": (1.0,)}, "scales"), ({"grid": (0, 1, 1)}, "grid"),
       ({"grid": (3, 2)}, "grid"), ({"grid": (3, 2.5, 1)}, "grid"), ({"search": "random", "k": 0}, "k")]


@pytest.mark.parametrize("kw,match", BAD)
def test_refusals_need_no_device(kw, match):
    from unidefense_amd.model import load_model
    m = load_model("UDR18")(num_classes=2).eval()
    for make in (lambda: SP.SpatialRunner(m, 2, 64, **kw), lambda: SP.spatial_runner(m, 2, 64, **kw), lambda: m.spatial_runner(2, 64, **kw)):
        with pytest.raises(ValueError, match=match):
            make()
    assert not m.__dict__.get("_ud_spatial_runners")
    free = {k: v for k, v in kw.items() if k in ("max_angle", "max_shift", "scales", "search", "grid", "k")}
    if free:
        with pytest.raises(ValueError, match=match):
            SP.spatial_candidates(64, **free)


def test_host_side_refusals():
    from unidefense_amd.model import load_model
    m = load_model("UDR18")(num_classes=2)
    with pytest.raises(ValueError, match="eval"):
        SP.SpatialRunner(m.train(), 2, 64)
    with pytest.raises(ValueError, match="cuda"):
        SP.SpatialRunner(m.eval(), 2, 64)
    with pytest.raises(ValueError, match="takes a UDEB4"):
        SP.SpatialRunner(torch.nn.Linear(2, 2), 2, 64)
    with pytest.raises(ValueError, match="cuda"):
        SP.warp(torch.zeros(1, 3, 16, 16))
    with pytest.raises(ValueError, match="border"):
        SP.warp(torch.zeros(1, 3, 16, 16), border="wrap")
    with pytest.raises(ValueError, match="batch"):
        SP.spatial_candidates(64, batch=0)


def test_entry_points_are_declared_exported_and_refuse_bad_arguments():
    from tests.test_abi_cpu import header
    from unidefense_amd import kernels as K
    from unidefense_amd import lib
    names = header().protos
    L = ctypes.CDLL(lib.LIB_PATH)
    for n in ("ud_warp_affine", "ud_spatial_control"):
        assert n in names and n in lib.EXPORTED and hasattr(L, n), n
        getattr(L, n).restype = ctypes.c_int
    for n in ("spatial_state", "warp_affine", "spatial_control"):
        assert callable(getattr(K, n)), n
    const = header().consts
    assert K.WARP_BORDER == {"reflect": 0, "edge": 1, "fill": 2}
    assert K.SPATIAL_I == {"k": 0, "best_k": 1, "row": 2} and K.SPATIAL_F == {"f_best": 0}
    assert {k: const[f"UD_WARP_{k.upper()}"] for k in K.WARP_BORDER} == K.WARP_BORDER and tuple(K.WARP_BORDER) == SP.BORDERS
    assert {k: const[f"UD_SPATIAL_I_{k.upper()}"] for k in K.SPATIAL_I} == K.SPATIAL_I
    assert K.SPATIAL_F == {"f_best": const["UD_SPATIAL_F_BEST"]}
    buf = (ctypes.c_float * 256)()
    a, b, t, i1, i2 = (ctypes.cast(ctypes.addressof(buf) + 64 * j, ctypes.c_void_p) for j in range(5))
    bad = [(None, b, t, i1, i2, 1, 16, 1, 0, None), (a, None, t, i1, i2, 1, 16, 1, 0, None), (a, b, None, i1, i2, 1, 16, 1, 0, None),
           (a, b, t, None, i2, 1, 16, 1, 0, None), (a, b, t, i1, None, 1, 16, 1, 0, None), (a, a, t, i1, i2, 1, 16, 1, 0, None),
           (a, b, t, i1, i2, 0, 16, 1, 0, None), (a, b, t, i1, i2, 65536, 16, 1, 0, None), (a, b, t, i1, i2, 1, 0, 1, 0, None),
           (a, b, t, i1, i2, 1, 40000, 1, 0, None), (a, b, t, i1, i2, 1, 16, 0, 0, None), (a, b, t, i1, i2, 1, 16, 1, 3, None),
           (a, b, t, i1, i2, 1, 16, 1, -1, None)]
    for args in bad:
        assert L.ud_warp_affine(*args) == -1000, args
    bad = [(None, i1, b, t, 4, 2, 0, None), (a, None, b, t, 4, 2, 0, None), (a, i1, None, t, 4, 2, 0, None), (a, i1, b, None, 4, 2, 0, None),
           (a, i1, b, t, 0, 2, 0, None), (a, i1, b, t, 4, 0, 0, None), (a, i1, b, t, 65536, 65536, 0, None), (None, None, None, None, 4, 2, 1, None)]
    for args in bad:
        assert L.ud_spatial_control(*args) == -1000, args
