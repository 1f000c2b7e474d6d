"""CPU: the adversarial patch's host side (unidefense_amd/patch.py, engine/evaluate.py: test_patch): placement_q16 on hand
values, every refusal without a device, the three entry points' argument tests, the numpy restatements' properties (exact
copies, x's bits outside, the adjoint identity), the PROOF that the gather's window holds every weighted (pixel, texel) pair,
what a smaller window loses, ref_patch_fit against a linear objective's closed form, the runner cache's key and the stage's
rules against stubs."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

from unidefense_amd import patch as PT
from unidefense_amd.engine import evaluate, metrics

Q = 65536


def _model():
    from unidefense_amd.model import load_model
    return load_model("UDR18")(num_classes=2).eval()


# ---- placement_q16 on hand values --------------------------------------------------------------------------------------------------
def test_placement_on_hand_values():
    ident = [Q, 0, 0, 0, Q, 0]
    # identity: the texture's centre t0 = 2 on the pixel (2, 2), no roll, one pixel per texel; reach = floor(1.425) + 2
    assert PT.placement_q16(5, (2, 2), 0.0, 1.0) == ident + ident + [3, 0, 0, 0]
    # an even side has its centre between texels: t0 = 1.5 on the pixel coordinate 1.5 is the identity again
    assert PT.placement_q16(4, (1.5, 1.5)) == ident + ident + [3, 0, 0, 0]
    # half a pixel to the right: the inverse map's column offset is -1/2 texel, the forward map's +1/2 pixel
    assert PT.placement_q16(5, (2.5, 2)) == [Q, 0, -Q // 2, 0, Q, 0, Q, 0, Q // 2, 0, Q, 0, 3, 0, 0, 0]
    # 90 degrees (x to the right, y down): texel column = pixel row - 0, texel row = 4 - pixel column
    assert PT.placement_q16(5, (2, 2), 90.0) == [0, Q, 0, -Q, 0, 4 * Q, 0, -Q, 4 * Q, Q, 0, 0, 3, 0, 0, 0]
    # P = 1: t0 = 0, the one texel sits on the centre
    assert PT.placement_q16(1, (3, 4)) == [Q, 0, -3 * Q, 0, Q, -4 * Q, Q, 0, 3 * Q, 0, Q, 4 * Q, 3, 0, 0, 0]
    # scale: the inverse map divides, the forward map multiplies; reach follows the scale
    row = PT.placement_q16(3, (10, 10), 0.0, 4.0)
    assert row[:6] == [Q // 4, 0, Q - 10 * Q // 4, 0, Q // 4, Q - 10 * Q // 4] and row[6:12] == [4 * Q, 0, 6 * Q, 0, 4 * Q, 6 * Q]
    assert row[12] == 7 and PT.placement_q16(3, (10, 10), 0.0, 0.25)[12] == 2 and PT.reach_of(4.0) == 7 and PT.reach_of(1.0) == 3
    assert all(type(v) is int for v in row) and len(row) == PT.ROW == 16
    assert PT.placement_q16(5, (2, 2), 180.0)[:6] == [-Q, 0, 4 * Q, 0, -Q, 4 * Q] and PT.placement_q16(5, (2, 2), -180.0)[:6] == [-Q, 0, 4 * Q, 0, -Q, 4 * Q]


def test_placement_and_table_refusals():
    for kw, text in (({"scale": 0.2}, "scale must be in [0.25, 4.0]"), ({"scale": 4.01}, "scale must be in"), ({"scale": float("nan")}, "scale must be in"),
                     ({"angle": float("inf")}, "finite"), ({"centre": (float("nan"), 0)}, "finite"), ({"centre": (1, 2, 3)}, "two finite"),
                     ({"centre": (40000, 0)}, "does not fit Q16"), ({"centre": (9000, 9000), "scale": 0.25}, "does not fit Q16")):
        with pytest.raises(ValueError, match=re.escape(text)):
            PT.placement_q16(**dict({"P": 5, "centre": (2, 2), "angle": 0.0, "scale": 1.0}, **kw))
    for P in (0, 257, 2.5, True):
        with pytest.raises(ValueError, match="patch must be an integer side"):
            PT.placement_q16(P, (2, 2))
    good = np.array([PT.placement_q16(5, (2, 2), 10.0, 4.0)], dtype=np.int64)
    assert PT.check_table(good).dtype == np.int32 and PT.check_table(torch.from_numpy(good)).shape == (1, 16)
    for col, v, text in ((12, 9, "reach"), (12, -1, "reach"), (13, 1, "reserved"), (15, -2, "reserved"), (2, 1 << 31, "int32")):
        bad = good.copy()
        bad[0, col] = v
        with pytest.raises(ValueError, match=text):
            PT.check_table(bad)
    with pytest.raises(ValueError, match="integers"):
        PT.check_table(good[:, :15])
    with pytest.raises(ValueError, match="integers"):
        PT.check_table(good.astype(np.float32))


def test_random_placements_stay_inside_the_region():
    g = torch.Generator().manual_seed(3)
    region = (0.25, 0.1, 1.0, 0.6)
    params, table = PT.patch_placements(200, 128, 16, max_angle=180.0, scales=(0.5, 2.0), region=region, generator=g)
    assert params.dtype == torch.float64 and tuple(params.shape) == (200, 4) and table.dtype == torch.int32 and tuple(table.shape) == (200, 16)
    cx, cy, ang, s = params.T
    rad = s * 16 / math.sqrt(2.0)
    assert bool((cx - rad >= 0.25 * 128 - 0.5).all()) and bool((cx + rad <= 128 - 0.5).all())
    assert bool((cy - rad >= 0.1 * 128 - 0.5).all()) and bool((cy + rad <= 0.6 * 128 - 0.5).all())
    assert bool((ang.abs() <= 180).all()) and float(ang.abs().max()) > 90 and 0.5 <= float(s.min()) < 0.6 and 1.9 < float(s.max()) <= 2.0
    for p, row in zip(params[:5].tolist(), table[:5].tolist()):
        assert row == PT.placement_q16(16, p[:2], p[2], p[3])
    again = PT.patch_placements(200, 128, 16, 180.0, (0.5, 2.0), region, torch.Generator().manual_seed(3))
    assert torch.equal(again[0], params) and torch.equal(again[1], table)
    one = PT.patch_placements(3, 64, 8, max_angle=0.0, scales=(1.0, 1.0), generator=g)[0]
    assert bool((one[:, 2] == 0).all()) and bool((one[:, 3] == 1).all())
    for kw, text in (({"scales": (0.1, 1.0)}, "scales must be"), ({"scales": (2.0, 1.0)}, "scales must be"), ({"max_angle": 181}, "max_angle"),
                     ({"region": (0.5, 0, 0.5, 1)}, "region must be"), ({"region": (0, 0, 1, 1.5)}, "region must be"),
                     ({"patch": 48}, "does not fit the region"), ({"region": (0.0, 0.0, 0.2, 1.0)}, "does not fit the region"), ({"n": 0}, "n must be")):
        with pytest.raises(ValueError, match=text):
            PT.patch_placements(**dict({"n": 2, "size": 64, "patch": 16, "scales": (1.0, 2.0)}, **kw))


def test_alpha_shapes():
    assert torch.equal(PT.patch_alpha(5), torch.ones(5, 5)) and PT.patch_alpha(5).dtype == torch.float32
    c = PT.patch_alpha(9, "circle")
    assert float(c[4, 4]) == 1.0 and float(c[4, 0]) == 1.0 and float(c[0, 0]) == 0.0 and torch.equal(c, c.t()) and torch.equal(c, c.flip(0))
    assert 0.0 < float(c[1, 1]) < 1.0                        # d = 3 sqrt(2) = 4.24: on the ramp between 4 and 5
    assert float(c[1, 1]) == pytest.approx(5.0 - 3 * math.sqrt(2.0), abs=1e-6)
    assert torch.equal(PT.patch_alpha(1, "circle"), torch.ones(1, 1))
    with pytest.raises(ValueError, match="shape must be one of"):
        PT.patch_alpha(5, "star")


# ---- refusals need no device ----------------------------------------------------------------------------------------------------------
BAD = [({"steps": 0}, "steps must be an integer >= 1"), ({"steps": 1.5}, "steps must be an integer >= 1"), ({"clip": (1.0, -1.0)}, "clip must be (lo, hi)"),
       ({"patch": 0}, "patch must be an integer side"), ({"patch": 300}, "patch must be an integer side"), ({"patch": 60}, "does not fit the region"),
       ({"scales": (0.2, 1.0)}, "scales must be"), ({"scales": (1.0, 5.0)}, "scales must be"), ({"max_angle": -1.0}, "max_angle must be"),
       ({"region": (0, 0, 1)}, "region must be"), ({"shape": "star"}, "shape must be one of ('square', 'circle')"),
       ({"alpha": torch.ones(4, 4)}, "alpha must be a [16, 16] tensor"), ({"alpha": torch.full((16, 16), 1.5)}, "alpha must lie in [0, 1]"),
       ({"beta": 0.0}, "beta must be > 0"), ({"beta": None}, "beta must be > 0"), ({"source": 2}, "source must be one of (None, 0, 1)"),
       ({"reduce": "sum"}, "reduce must be None or a callable"), ({"step": float("nan")}, "step must be finite"),
       ({"precision": "bf16"}, "precision"), ({"precision": "fp16"}, "fp16"), ({"grad_scale": 3.0}, "grad_scale")]


@pytest.mark.parametrize("kw,text", BAD)
def test_refusals_need_no_device(kw, text):
    m = _model()
    kw = dict({"patch": 16}, **kw)
    for make in (lambda: PT.PatchRunner(m, 2, 64, **kw), lambda: PT.patch_runner(m, 2, 64, **kw), lambda: m.patch_runner(2, 64, **kw)):
        with pytest.raises(ValueError, match=re.escape(text)):
            make()
    assert not m.__dict__.get("_ud_patch_runners")


def test_host_side_refusals_and_defaults():
    from unidefense_amd.model import load_model
    m = load_model("UDR18")(num_classes=2)
    with pytest.raises(ValueError, match="eval"):
        PT.PatchRunner(m.train(), 2, 64)
    with pytest.raises(ValueError, match="cuda"):            # every argument passed: only the device is missing
        PT.PatchRunner(m.eval(), 2, 64, patch=8, shape="circle", steps=3, step=0.1, max_angle=30.0, scales=(0.5, 2.0),
                       region=(0.1, 0.1, 0.9, 0.9), beta=1.0, source=1, reduce=lambda g: None)
    with pytest.raises(ValueError, match="takes a UDEB4"):
        PT.PatchRunner(torch.nn.Linear(2, 2), 2, 64)
    for name in ("UDEB4", "UDR18", "UDR50"):
        assert callable(getattr(load_model(name), "patch_runner")) and callable(getattr(load_model(name), "universal_runner"))
    assert PT.resolve_patch_step((-1.0, 1.0)) == 2.0 / 64 and PT.resolve_patch_step((0.0, 1.0), None) == 1.0 / 64 and PT.resolve_patch_step((-1, 1), 0.25) == 0.25
    a = PT._patch_arguments(4, 128)
    assert list(a) == ["batch", "size", "patch", "shape", "alpha", "steps", "step", "max_angle", "scales", "region", "beta", "source", "clip",
                       "precision", "grad_scale", "reduce"]
    assert (a["patch"], a["shape"], a["alpha"], a["steps"], a["step"], a["max_angle"], a["scales"], a["region"], a["beta"], a["source"], a["clip"],
            a["precision"], a["reduce"]) == (32, "square", None, 1, None, 15.0, (0.8, 1.25), (0.0, 0.0, 1.0, 1.0), math.inf, None, (-1.0, 1.0), "fp32", None)
    with pytest.raises(ValueError, match="cuda"):
        PT.paste(torch.zeros(1, 3, 8, 8), torch.zeros(3, 2, 2), [PT.placement_q16(2, (3, 3))])


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_refuse_bad_arguments():
    from tests.test_abi_cpu import header
    from unidefense_amd import kernels as K
    from unidefense_amd import lib
    h = header()
    L = ctypes.CDLL(lib.LIB_PATH)
    names = ("ud_patch_paste", "ud_patch_grad", "ud_patch_update")
    for n in names:
        assert n in h.protos and n in lib.EXPORTED and hasattr(L, n), n
        assert h.protos[n][0] is ctypes.c_int, n
        fn = getattr(L, n)
        fn.restype, fn.argtypes = ctypes.c_int, [t for t, _ in h.protos[n][1]]
    assert sorted(n for n in h.protos if n.startswith("ud_patch")) == sorted(names)              # no workspace query: there is no workspace
    for n in ("patch_paste", "patch_grad", "patch_update"):
        assert callable(getattr(K, n)), n
    assert h.consts["UD_PATCH_ROW"] == K.PATCH_ROW == PT.ROW == 16 and h.consts["UD_PATCH_MAX_REACH"] == K.PATCH_MAX_REACH == PT.MAX_REACH == 8
    buf = (ctypes.c_double * 64)()
    a, b, c, d, e, f = (ctypes.cast(ctypes.addressof(buf) + 64 * j, ctypes.c_void_p) for j in range(6))
    nan = float("nan")
    ok = (a, b, c, d, e, 2, f, 4, 16, 5, -1.0, 1.0, None)             # (x, patch, alpha, table, k, rows, out, N, S, P, lo, hi)
    bad = [ok[:i] + (None,) + ok[i + 1:] for i in (0, 1, 2, 3, 4, 6)]
    bad += [ok[:6] + (a,) + ok[7:]]                                   # out == x
    bad += [ok[:5] + (rows,) + ok[6:] for rows in (0, -1)]
    bad += [ok[:7] + t + (None,) for t in ((0, 16, 5, -1.0, 1.0), (65536, 16, 5, -1.0, 1.0), (4, 1, 5, -1.0, 1.0), (4, 32769, 5, -1.0, 1.0),
                                           (4, 16, 0, -1.0, 1.0), (4, 16, 257, -1.0, 1.0), (4, 16, 5, 1.0, -1.0), (4, 16, 5, nan, 1.0),
                                           (4, 16, 5, -1.0, nan))]
    for args in bad:
        assert L.ud_patch_paste(*args) == -1000, args
    ok = (a, b, c, d, 2, e, 4, 16, 5, None)                           # (g, alpha, table, k, rows, gp, N, S, P)
    bad = [ok[:i] + (None,) + ok[i + 1:] for i in (0, 1, 2, 3, 5)]
    bad += [ok[:5] + (a,) + ok[6:], ok[:4] + (0,) + ok[5:]]           # gp == g; rows < 1
    bad += [ok[:6] + t + (None,) for t in ((0, 16, 5), (65536, 16, 5), (4, 1, 5), (4, 32769, 5), (4, 16, 0), (4, 16, 257))]
    for args in bad:
        assert L.ud_patch_grad(*args) == -1000, args
    ok = (a, b, 75, 0.1, -1.0, 1.0, None)                             # (patch, gsum, per, step, lo, hi)
    bad = [ok[:i] + (None,) + ok[i + 1:] for i in (0, 1)] + [(a, a) + ok[2:]]
    bad += [ok[:2] + t + (None,) for t in ((0, 0.1, -1.0, 1.0), (-3, 0.1, -1.0, 1.0), (3 * 256 * 256 + 1, 0.1, -1.0, 1.0), (75, nan, -1.0, 1.0),
                                           (75, 0.1, 1.0, -1.0), (75, 0.1, nan, 1.0), (75, 0.1, -1.0, nan))]
    for args in bad:
        assert L.ud_patch_update(*args) == -1000, args


def test_wrappers_refuse_cpu_tensors():
    from unidefense_amd import kernels as K
    x, p, al = torch.zeros(2, 3, 8, 8), torch.zeros(3, 4, 4), torch.ones(4, 4)
    t, k = torch.zeros(1, 2, 16, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    for call in (lambda: K.patch_paste(x, p, al, t, k, x.clone(), -1, 1), lambda: K.patch_grad(x, al, t, k, torch.zeros(2, 3, 4, 4)),
                 lambda: K.patch_update(p, p.clone(), 0.1, -1, 1)):
        with pytest.raises(ValueError, match="CUDA"):
            call()


# ---- the restatements -------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_ref_paste_copies_exactly_and_leaves_the_rest():
    rng = np.random.default_rng(0)
    S, P = 12, 5
    x = rng.uniform(-1, 1, (2, 3, S, S)).astype(np.float32)
    x[0, 0, 0, 0] = 1.5                                              # outside the clip: the paste does not clamp what it does not touch
    patch = rng.uniform(-1, 1, (3, P, P)).astype(np.float32)
    ones = PT.patch_alpha(P)
    # integer-aligned at scale 1: texel (i, j) lands on the pixel (i + 3, j + 4), weight exactly 1
    table = np.array([PT.placement_q16(P, (6, 5)), PT.placement_q16(P, (100, -50))])
    out = PT.ref_patch_paste(x, patch, ones, table)
    assert out.dtype == np.float32 and np.array_equal(_bits(out[0, :, 3:8, 4:9]), _bits(patch))
    rest = np.ones((S, S), bool)
    rest[3:8, 4:9] = False
    assert np.array_equal(_bits(out[0][:, rest]), _bits(x[0][:, rest])) and out[0, 0, 0, 0] == np.float32(1.5)
    assert np.array_equal(_bits(out[1]), _bits(x[1]))               # a patch fully outside the image: x bit for bit
    # rolled by 90 and 180 degrees about an integer centre: exact copies of the rotated texture
    for angle, want in ((90.0, np.rot90(patch, -1, (1, 2))), (180.0, patch[:, ::-1, ::-1])):
        out = PT.ref_patch_paste(x[:1], patch, ones, [PT.placement_q16(P, (6, 5), angle)])
        assert np.array_equal(_bits(out[0, :, 3:8, 4:9]), _bits(want)), angle
    # half a pixel: the mean of two neighbours inside, a half-covered blend with x on the edge column
    out = PT.ref_patch_paste(x[:1], patch, ones, [PT.placement_q16(P, (6.5, 5))])
    assert np.array_equal(out[0, :, 3:8, 5:9], np.float32(0.5) * patch[:, :, :-1] + np.float32(0.5) * patch[:, :, 1:])
    assert np.array_equal(out[0, :, 3:8, 4], np.float32(0.5) * x[0, :, 3:8, 4] + np.float32(0.5) * patch[:, :, 0])
    # alpha: zero coverage keeps x's bits, a NaN texel shows only where it has weight, the result stays inside the clip
    circle = PT.patch_alpha(P, "circle")
    circle[0, 0] = 0.0                                               # (at side 5 the corner still has 0.17)
    bad = patch.copy()
    bad[1, 2, 2] = np.nan
    out = PT.ref_patch_paste(x[:1], bad * 3, circle, [PT.placement_q16(P, (6, 5))])
    assert np.array_equal(_bits(out[0, :, 3, 4]), _bits(x[0, :, 3, 4])) and float(circle[0, 0]) == 0.0
    assert int(np.isnan(out).sum()) == 1 and np.isnan(out[0, 1, 5, 6])
    assert np.nanmax(out[0, :, 3:8, 4:9]) <= 1.0 and np.nanmin(out[0, :, 3:8, 4:9]) >= -1.0
    # x is only read
    keep = x.copy()
    PT.ref_patch_paste(x, patch, ones, table)
    assert np.array_equal(_bits(x), _bits(keep))


# the placements of the window proof: the issue's ranges, their ends included (scale 0.25 and 4, +-180 degrees, centres outside)
def _proof_cases():
    rng = np.random.default_rng(7)
    cases = [(20, 5, (9.3, 7.7), 17.0, 4.0), (20, 5, (9.3, 7.7), 17.0, 0.25), (33, 8, (16, 16), 180.0, 4.0), (33, 8, (16.5, 15.5), -180.0, 0.25),
             (8, 1, (-3.5, 2.0), 45.0, 4.0), (24, 33, (27.9, -4.0), 45.0, 0.25), (16, 4, (20.0, 19.99), -135.0, 2.83), (96, 33, (48, 48), 30.0, 1.0)]
    for _ in range(100):
        S, P = int(rng.integers(8, 97)), int(rng.integers(1, 34))
        s = float(rng.choice([0.25, 4.0, rng.uniform(0.25, 4.0), rng.uniform(0.25, 1.0)]))
        cases.append((S, P, tuple(rng.uniform(-4.0, S + 3.0, 2)), float(rng.choice([180.0, -180.0, 90.0, rng.uniform(-180, 180)])), s))
    return cases


def test_window_holds_every_weighted_pair():
    """The proof behind ud_patch_grad's gather: for every placement tried, NONE skipped, every (pixel, texel) pair with a
    non-zero weight lies inside the texel's window, with at least one pixel to spare, and reach <= 7 < UD_PATCH_MAX_REACH."""
    pairs = 0
    for n, (S, P, centre, angle, scale) in enumerate(_proof_cases()):
        row = PT.placement_q16(P, centre, angle, scale)
        assert 2 <= row[12] <= 7
        r, c = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
        for i, j, om, present in PT.ref_patch_taps(row, PT.patch_alpha(P, "circle" if n % 2 else "square"), S):
            pc, pr = (row[6] * j + row[7] * i + row[8] + 32768) >> 16, (row[9] * j + row[10] * i + row[11] + 32768) >> 16
            far = np.maximum(np.abs(r - pr), np.abs(c - pc))[present]
            pairs += far.size
            assert far.size == 0 or int(far.max()) <= row[12] - 1, (S, P, centre, angle, scale, int(far.max()), row[12])
    assert pairs > 100000


def _grad_case(S, P, rows, seed, shape="circle"):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((len(rows), 3, S, S)).astype(np.float32)
    return g, PT.patch_alpha(P, shape), np.array(rows, dtype=np.int32)


def test_adjoint_identity_in_float64():
    """<paste(0, p), g> = <p, ref_patch_grad(g)> with the clip out of reach, to 1e-12 relative"""
    S, P = 20, 5
    rows = [PT.placement_q16(P, (9.3, 7.7), 17.0, 1.7), PT.placement_q16(P, (1.0, 1.5), -30.0, 0.6), PT.placement_q16(P, (10, 10), 77.0, 4.0)]
    g, alpha, table = _grad_case(S, P, rows, 1)
    p = np.random.default_rng(2).standard_normal((3, P, P))
    lhs = 0.0
    for n in range(len(rows)):                                       # the paste of p into zeros, in float64 with the paste's own weights
        pasted = np.zeros((3, S, S))
        for i, j, om, present in PT.ref_patch_taps(table[n], alpha, S):
            pasted += np.where(present, om.astype(np.float64), 0.0) * p[:, i, j]
        lhs += float((pasted * g[n]).sum())
        # and that IS the float32 paste, up to its roundings
        f32 = PT.ref_patch_paste(np.zeros((1, 3, S, S), np.float32), p.astype(np.float32), alpha, table[n:n + 1], -1e9, 1e9)[0]
        assert np.abs(f32 - pasted).max() <= 1e-5
    gp, mag = PT.ref_patch_grad(g, alpha, table, magnitude=True)
    rhs = float((gp.sum(0) * p).sum())
    assert gp.dtype == np.float64 and abs(lhs - rhs) <= 1e-12 * abs(lhs) and abs(lhs) > 1e-3
    assert np.all(mag >= np.abs(gp)) and np.array_equal(gp[:, :, alpha.numpy() == 0], np.zeros_like(gp[:, :, alpha.numpy() == 0]))


def _worst(got, ref, mag):
    """the GPU file's bar: |got - ref| <= 2^-23 |ref| + 2^-40 sum |omega g|; the largest ratio of the two sides"""
    bound = 2.0 ** -23 * np.abs(ref) + 2.0 ** -40 * mag
    err = np.abs(got.astype(np.float64) - ref)
    assert np.all(err[bound == 0] == 0)
    return float((err[bound > 0] / bound[bound > 0]).max()) if np.any(bound > 0) else 0.0


def test_gather_restatement_meets_the_bar_and_a_smaller_window_does_not():
    S, P = 20, 5
    rows = [PT.placement_q16(P, (9.3, 7.7), 45.0, 4.0), PT.placement_q16(P, (9.3, 7.7), 17.0, 0.25), PT.placement_q16(P, (9.5, 9.5), 17.0, 1.7),
            PT.placement_q16(P, (0.0, 19.0), 45.0, 1.0), PT.placement_q16(P, (60.0, 60.0), 0.0, 1.0)]
    g, alpha, table = _grad_case(S, P, rows, 3)
    ref, mag = PT.ref_patch_grad(g, alpha, table, magnitude=True)
    got = PT.ref_patch_grad_gather(g, alpha, table)
    assert got.dtype == np.float32 and _worst(got, ref, mag) <= 1.0
    assert not got[4].any() and not ref[4].any()                      # fully outside: zeros
    assert np.array_equal(_bits(got), _bits(PT.ref_patch_grad_gather(g, alpha, table)))
    # scale 4 rolled by 45 degrees: a texel weighs pixels up to 4 sqrt(2) + 1/2 = 6.2 away; a window of reach - 2 = 5 cuts them off
    short = PT.ref_patch_grad_gather(g[:1], alpha, table[:1], shrink=2)
    worst = _worst(short, ref[:1], mag[:1])
    assert worst > 1e3, worst
    assert _worst(PT.ref_patch_grad_gather(g[:1], alpha, table[:1], shrink=1), ref[:1], mag[:1]) <= 1.0     # the spare pixel


def test_ref_update_rule():
    p = np.array([0.0, 0.9, -0.9, 0.3, 0.3, 1.0, 0.2])
    gs = np.array([1.0, 2.0, -3.0, 0.0, -0.0, 5.0, np.nan])
    got = PT.ref_patch_update(p, gs, 0.25, -1.0, 1.0)
    assert got.dtype == np.float64 and got[:6].tolist() == [0.25, 1.0, -1.0, 0.3, 0.3, 1.0] and np.isnan(got[6])


def test_ref_fit_reaches_the_closed_form_of_a_linear_objective():
    """f_n = <c_n, x_adv_n>: the gradient is c whatever the patch, so with ONE placement per sample held over the iterations
    every texel under coverage walks to the clip face of the sign of its summed adjoint, and stays there"""
    S, P, N, steps = 16, 5, 3, 9
    rng = np.random.default_rng(5)
    c = rng.standard_normal((N, 3, S, S))
    x = rng.uniform(-1, 1, (N, 3, S, S)).astype(np.float32)
    alpha = PT.patch_alpha(P, "circle")
    rows = np.array([PT.placement_q16(P, (7.3, 8.1), 20.0, 1.3), PT.placement_q16(P, (4.0, 4.0), -10.0, 0.8), PT.placement_q16(P, (30.0, 4.0), 0.0, 1.0)])
    tables = np.broadcast_to(rows, (steps + 1, N, 16))
    seen = []

    def grad(xa):
        assert xa.dtype == np.float32 and xa.shape == x.shape
        seen.append(xa.copy())
        return c, (c * xa).sum((1, 2, 3))

    patch, x_adv = PT.ref_patch_fit(grad, x, np.zeros((3, P, P)), alpha, tables, step=0.25)
    gsum = PT.ref_patch_grad(c, alpha, rows).sum(0)
    want = np.sign(gsum)                                              # 9 steps of 1/4 from 0 reach +-1
    assert len(seen) == steps and np.array_equal(patch, want) and np.all(patch[:, alpha.numpy() == 0] == 0) and np.any(want != 0)
    assert np.array_equal(_bits(x_adv), _bits(PT.ref_patch_paste(x, want, alpha, rows))) and np.array_equal(_bits(x_adv[2]), _bits(x[2]))
    assert np.array_equal(_bits(seen[0]), _bits(PT.ref_patch_paste(x, np.zeros((3, P, P)), alpha, rows)))
    # who steers: only sample 1 (source), or nobody (beta below every f): the sign of that sample's adjoint, or no move
    y = np.array([0, 1, 0])
    only = PT.ref_patch_fit(grad, x, np.zeros((3, P, P)), alpha, tables, step=0.25, source=1, y=y)[0]
    assert np.array_equal(only, np.sign(PT.ref_patch_grad(c, alpha, rows)[1]))
    none = PT.ref_patch_fit(grad, x, np.full((3, P, P), 0.5), alpha, tables, step=0.25, beta=-1e9)[0]
    assert np.all(none == 0.5)


# ---- the cache's key ----------------------------------------------------------------------------------------------------------------------
def test_cache_key(monkeypatch):
    made = []

    class Stub:
        def __init__(self, model, *args):
            made.append(args)
            self.P, self.alpha = args[2], torch.zeros(args[2], args[2])

    monkeypatch.setattr(PT, "PatchRunner", Stub)
    m = _model()

    def hook(gsum):
        return None

    r = PT.patch_runner(m, 4, 128)
    assert PT.patch_runner(m, 4, 128) is r and m.patch_runner(4, 128, patch=32, shape="square", steps=1) is r
    assert PT.patch_runner(m, 4, 128, 32, "square", None, 1, None, 15.0, [0.8, 1.25], [0.0, 0.0, 1.0, 1.0]) is r and len(made) == 1
    others = [PT.patch_runner(m, 4, 128, **kw) for kw in ({"patch": 16}, {"shape": "circle"}, {"scales": (1.0, 1.0)}, {"source": 1}, {"reduce": hook})]
    assert len({id(o) for o in others + [r]}) == 6 and len(made) == 6
    assert PT.patch_runner(m, 4, 128, reduce=hook) is others[4] and made[5][-1] is hook          # a callable is keyed by identity
    # an explicit alpha is contents: one runner for the other arguments, refilled on every fetch, never aliased
    a1, a2 = torch.full((32, 32), 0.25), torch.full((32, 32), 0.75)
    ra = PT.patch_runner(m, 4, 128, alpha=a1)
    assert ra is not r and made[-1][4] is a1
    assert PT.patch_runner(m, 4, 128, alpha=a2) is ra and torch.equal(ra.alpha, a2) and ra.alpha.data_ptr() != a2.data_ptr()
    from unidefense_amd.infer import _MAX_RUNNERS
    assert len(m.__dict__["_ud_patch_runners"]) <= _MAX_RUNNERS
    assert not any(k.startswith("_ud_") and k != "_ud_patch_runners" for k in m.__dict__)        # a dictionary of its own


# ---- the stage against stubs ----------------------------------------------------------------------------------------------------------------
DEV = torch.device("cpu")
P8 = 4


def logits(x):
    return torch.stack([x[:, :1].mean((1, 2, 3)), x[:, 1:].mean((1, 2, 3))], 1) * 8.0


def p0(x):
    return torch.softmax(logits(x), 1)[:, 0]


class Batches:
    """seeded batches of 2 real + 2 fake 3x8x8 images per step; .steps logs the steps drawn"""

    def __init__(self):
        self.steps = []

    def __call__(self, step, batch, size, device):
        self.steps.append(step)
        g = torch.Generator().manual_seed(100 + step)
        xr, xf = (torch.rand(batch, 3, size, size, generator=g) * 2 - 1 for _ in range(2))
        return xr, torch.zeros(batch, dtype=torch.long), xf, torch.ones(batch, dtype=torch.long)

    @staticmethod
    def of(steps, batch=2, size=8):
        parts = [Batches()(s, batch, size, DEV) for s in steps]
        return torch.cat([torch.cat([p[0], p[2]]) for p in parts]), torch.cat([torch.cat([p[1], p[3]]) for p in parts])


def host_paste(x, patch, table, alpha=None, clip=(-1.0, 1.0), out=None):
    return torch.from_numpy(PT.ref_patch_paste(x, patch, torch.ones(P8, P8) if alpha is None else alpha, table, clip[0], clip[1]))


class StubRunner:
    """the patch's channel 0 grows by 0.4 per call (the fit is visible in the scores); counted: call c counts c % 3 samples;
    every call consumes one draw of the stage's generator, as the real runner's placements do"""

    def __init__(self, net, kwargs):
        self.net, self.calls = net, 0
        self.args = dict({"method": "patch", "patch": P8, "shape": "square", "steps": 1, "max_angle": 15.0, "scales": (1.0, 1.25),
                          "region": (0.0, 0.0, 1.0, 1.0), "clip": (-1.0, 1.0), "area": P8 ** 2 * 1.125 ** 2 / 64.0}, **kwargs)
        self.patch, self.alpha = torch.zeros(3, P8, P8), PT.patch_alpha(P8, "circle")
        self.counted = torch.zeros(1, 4, dtype=torch.int32)

    def reset(self, value=0.0):
        self.net.log.append("reset")
        self.patch.fill_(value)

    def __call__(self, x, y, generator=None):
        self.net.log.append(("fit", float(x.sum()), float(torch.rand(1, generator=generator))))
        self.calls += 1
        self.patch[0] -= 0.4
        self.counted.zero_()
        self.counted[0, :self.calls % 3] = 1
        return x

    def apply(self, x, generator=None, table=None):
        assert table is not None and generator is None               # the stage brings the placements: the same for all four columns
        self.net.log.append("apply")
        return host_paste(x, self.patch, table, self.alpha)


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.log, self.runner = [], None

    def forward(self, x):
        self.log.append("forward")
        return {"cls_out": logits(x)}

    def patch_runner(self, n, size, patch=P8, steps=1, reduce=None):
        self.log.append(("patch_runner", n, size))
        if self.runner is None:
            self.runner = StubRunner(self, {"patch": patch, "steps": steps})
        return self.runner


def make():
    net, it = Net(), Batches()
    return evaluate.Evaluator(net, net, it, 2, 8, DEV), net, it


def expected(scores, labels):
    sc, lb = scores.numpy(), labels.numpy()
    ret = {"scores": scores, "labels": labels, "acc": float(np.mean((sc < 0.5).astype(int) == lb))}
    ret.update(metrics.cal_metrics(lb, sc, threshold=0.5))
    return ret


def same(got, want):
    assert set(got) == set(want)
    for k, v in want.items():
        assert torch.equal(got[k], v) if torch.is_tensor(v) else got[k] == v, k


def test_stage_fit_then_held_out_four_ways(monkeypatch):
    gathered = []
    real = metrics.gather_scores
    monkeypatch.setattr(metrics, "gather_scores", lambda s, lb: gathered.append(s) or real(s, lb))
    ev, net, it = make()
    given = {"patch": P8, "steps": 1, "seed": 9}
    got = ev.test_patch(2, 3, 2, given, paste=host_paste)
    assert given == {"patch": P8, "steps": 1, "seed": 9}                          # the caller's dict is not consumed
    assert it.steps == [1, 2, 3, 1, 2, 3, 4, 5]                                  # the fit, epochs times over, then the held-out steps
    g = torch.Generator().manual_seed(9)                                         # ONE seeded CPU generator: the fit's draws, the control, the placements
    fits = [(float(Batches.of([s])[0].sum()), float(torch.rand(1, generator=g))) for s in (1, 2, 3, 1, 2, 3)]
    assert net.log == [("patch_runner", 4, 8), "reset"] + [("fit",) + f for f in fits] + ["forward", "apply", "forward", "forward", "forward"] * 2
    random = torch.rand(3, P8, P8, generator=g) * 2.0 - 1.0
    middle = torch.zeros(3, P8, P8)
    texture = torch.zeros(3, P8, P8)
    texture[0] = -0.4 * 6
    x, y = Batches.of([4, 5])
    tables = [PT.patch_placements(4, 8, P8, 15.0, (1.0, 1.25), (0.0, 0.0, 1.0, 1.0), g)[1] for _ in range(2)]
    alpha = net.runner.alpha

    def pasted(p):
        return torch.cat([host_paste(x[:4], p, tables[0], alpha), host_paste(x[4:], p, tables[1], alpha)])

    want = {"clean": p0(x), "adv": p0(pasted(net.runner.patch)), "random": p0(pasted(random)), "occlusion": p0(pasted(middle))}
    assert set(got) == {"clean", "adv", "random", "occlusion", "attack"}
    for name in want:
        same(got[name], expected(want[name], y))
    assert len(gathered) == 4 and all(torch.equal(a, want[k]) for a, k in zip(gathered, ("clean", "adv", "random", "occlusion")))
    assert not torch.equal(want["adv"], want["clean"]) and not torch.equal(want["random"], want["occlusion"])
    a = got["attack"]
    assert set(a) == {"method", "patch", "shape", "steps", "max_angle", "scales", "region", "clip", "area", "texture", "fooled", "fooled_random",
                      "fooled_occlusion", "fit_counted"}
    assert (a["method"], a["patch"], a["steps"], a["area"]) == ("patch", P8, 1, 16 * 1.125 ** 2 / 64.0)
    assert a["texture"].device.type == "cpu" and torch.equal(a["texture"], net.runner.patch) and torch.allclose(a["texture"], texture)
    assert a["fit_counted"] == [1, 2, 0, 1, 2, 0] and all(type(c) is int for c in a["fit_counted"])
    right = (want["clean"] < 0.5).long() == y
    for key, name in (("fooled", "adv"), ("fooled_random", "random"), ("fooled_occlusion", "occlusion")):
        flipped = ((want[name] < 0.5).long() != y) & right
        assert type(a[key]) is float and a[key] == float(flipped.sum()) / float(right.sum())
    assert 0 < int(right.sum()) < 8 and a["fooled"] > 0                          # the stub's patch flips some


def test_stage_fooled_arithmetic_on_hand_made_scores(monkeypatch):
    """labels 0 (real: right where the score >= 0.5) and 1 (fake: right where it is < 0.5)"""
    scores = {"clean": torch.tensor([0.9, 0.8, 0.4, 0.7, 0.2, 0.1, 0.6, 0.3]),          # right: 0 1 3 | 4 5 7  (2 and 6 are wrong)
              "adv": torch.tensor([0.4, 0.8, 0.9, 0.3, 0.7, 0.1, 0.1, 0.6]),            # flips 0, 3, 4, 7 of the six
              "random": torch.tensor([0.9, 0.8, 0.9, 0.7, 0.2, 0.6, 0.6, 0.3]),         # flips 5
              "occlusion": torch.tensor([0.9, 0.8, 0.9, 0.7, 0.2, 0.1, 0.1, 0.3])}      # flips none
    labels = torch.tensor([0, 0, 0, 0, 1, 1, 1, 1])
    ev, net, it = make()
    monkeypatch.setattr(ev, "run", lambda n, body, first=1: {k: (v, labels) for k, v in scores.items()})
    a = ev.test_patch(2, 1, 1, {"seed": 1}, paste=host_paste)["attack"]
    assert (a["fooled"], a["fooled_random"], a["fooled_occlusion"]) == (4 / 6, 1 / 6, 0.0)
    scores["clean"] = torch.tensor([0.1, 0.1, 0.1, 0.1, 0.9, 0.9, 0.9, 0.9])            # nothing classified correctly: NaN
    a = ev.test_patch(2, 1, 1, None, paste=host_paste)["attack"]
    assert all(a[k] != a[k] for k in ("fooled", "fooled_random", "fooled_occlusion"))


def test_stage_refusals_fire_before_any_batch():
    ev, net, it = make()
    with pytest.raises(ValueError, match="^patch takes PatchRunner's keyword arguments and 'seed': .*stepz"):
        ev.test_patch(1, 1, 1, {"stepz": 3})
    for kw, text in (({"batches": 0}, "batches must be an integer >= 1"), ({"fit_batches": 0}, "fit_batches must be an integer >= 1"),
                     ({"epochs": 1.5}, "epochs must be an integer >= 1")):
        with pytest.raises(ValueError, match=text):
            ev.test_patch(**dict({"batches": 1, "fit_batches": 1, "epochs": 1, "patch": None}, **kw))
    assert it.steps == [] and "forward" not in net.log and net.runner is None
    # the real accessor's refusals are ValueErrors already: they pass through, before any batch
    ev = evaluate.Evaluator(_model(), _model(), it, 2, 8, DEV)
    with pytest.raises(ValueError, match="does not fit the region"):
        ev.test_patch(1, 1, 1, None)                                             # the default side 32 in an 8-pixel image
    with pytest.raises(ValueError, match="patch takes PatchRunner's keyword arguments and 'seed'"):
        ev.test_patch(1, 1, 1, {"patch": 4, "eps": 0.1})
    assert it.steps == []
