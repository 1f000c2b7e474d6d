"""CPU: the frequency-band attack's host side (unidefense_amd/band.py, engine/evaluate.py: test_band): the DCT matrix and the band
masks, the float64 restatements on a closed form, the three-dot identity, the parity bar's power against subtly wrong transforms,
every refusal without a device, the runner cache's key, the entry points' argument tests and the stage's rules against stubs."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

from tests.parity import bar_of
from unidefense_amd import band as BD
from unidefense_amd.engine import evaluate, metrics

EPS = 1.0


def _model():
    from unidefense_amd.model import load_model
    return load_model("UDR18")(num_classes=2).eval()


# ---- the matrix and the masks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 3, 8, 95, 128])
def test_dct_matrix_is_orthonormal(S):
    D = BD.dct_matrix(S)
    assert D.dtype == torch.float64 and tuple(D.shape) == (S, S)
    assert float((D @ D.t() - torch.eye(S, dtype=torch.float64)).abs().max()) <= 1e-13
    assert float((D[0] - math.sqrt(1.0 / S)).abs().max()) == 0.0
    i = np.arange(S)
    want = np.sqrt(2.0 / S) * np.cos(np.pi * (2 * i[None, :] + 1) * i[:, None] / (2.0 * S))
    want[0] = np.sqrt(1.0 / S)
    assert np.abs(D.numpy() - want).max() <= 1e-15
    try:
        import scipy.fft
    except ImportError:
        return
    assert np.abs(D.numpy() - scipy.fft.dct(np.eye(S), norm="ortho", axis=0)).max() <= 1e-14


@pytest.mark.parametrize("shape", BD.SHAPES)
@pytest.mark.parametrize("S", [8, 95])
def test_default_bands_partition_the_plane(S, shape):
    masks = [BD.band_mask(S, lo, hi, shape) for lo, hi in BD.DEFAULT_BANDS]
    assert all(m.dtype == torch.float32 and tuple(m.shape) == (S, S) and set(m.unique().tolist()) <= {0.0, 1.0} for m in masks)
    assert torch.equal(sum(masks), torch.ones(S, S))                                 # exactly: every coefficient in one band
    assert [float(m[0, 0]) for m in masks] == [1.0, 0.0, 0.0, 0.0]                    # DC is in the band exactly when lo == 0
    assert all(float(m.sum()) > 0 for m in masks)
    assert torch.equal(BD.band_mask(S, 0.0, None, shape), torch.ones(S, S))
    u = torch.arange(S, dtype=torch.float64)
    r = torch.sqrt(u[:, None] ** 2 + u[None, :] ** 2) / S if shape == "radial" else torch.maximum(u[:, None], u[None, :]) / S
    assert torch.equal(masks[1], ((r >= 1 / 8) & (r < 1 / 4)).float())
    assert BD.DEFAULT_BANDS == ((0.0, 1 / 8), (1 / 8, 1 / 4), (1 / 4, 1 / 2), (1 / 2, None))


@pytest.mark.parametrize("args,text", [((8, 0.5, 0.25), "lo < hi"), ((8, 0.25, 0.25), "lo < hi"), ((8, -0.1, 0.5), "lo must be a finite number >= 0"),
                                       ((8, float("nan")), "lo must be"), ((8, 0.0, 0.5, "ring"), "shape must be one of ('radial', 'square')"),
                                       ((1, 0.0), "size must be an integer >= 2")])
def test_band_mask_refusals(args, text):
    with pytest.raises(ValueError, match=re.escape(text)):
        BD.band_mask(*args)


# ---- the restatements ---------------------------------------------------------------------------------------------------------------------
def test_ref_dct2_is_the_definition_and_inverts():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 12, 12, generator=g, dtype=torch.float64)
    D = BD.dct_matrix(12)
    y = BD.ref_dct2(x)
    assert torch.equal(y[1, 2], D @ x[1, 2] @ D.t())
    assert float((BD.ref_dct2(y, inverse=True) - x).abs().max()) <= 1e-13
    assert float((y.flatten(1).norm(dim=1) - x.flatten(1).norm(dim=1)).abs().max()) <= 1e-12       # |dct2(x)|_2 = |x|_2
    m = BD.band_mask(12, 0.25, 0.5)
    assert torch.equal(BD.ref_dct2(x, m), y * m) and torch.equal(BD.ref_dct2(y, m, inverse=True), D.t() @ (y * m) @ D)
    assert float(y[0, 0, 0, 0] - x[0, 0].sum() / 12) <= 1e-13                         # DC: the mean times S


@pytest.mark.parametrize("shape", BD.SHAPES)
@pytest.mark.parametrize("S,band", [(8, (0.125, 0.5)), (19, (0.0, 0.25)), (19, (0.5, None))])
def test_ref_attack_converges_to_the_closed_form(S, band, shape):
    """f = <c, x>, clip inactive: the iterate goes to eps P c / |P c|_2, P = band_project"""
    g = torch.Generator().manual_seed(S)
    n, eps, step = 2, 0.3, 0.04
    c = torch.randn(n, 3, S, S, generator=g, dtype=torch.float64)
    x = torch.randn(n, 3, S, S, generator=g, dtype=torch.float64) * 0.1
    mask = BD.band_mask(S, *band, shape)

    def fg(xa, y):
        return (c * xa).flatten(1).sum(1), c.clone()

    ret = BD.ref_band_attack(fg, x, None, mask, eps, 12, step, clip=(-10.0, 10.0))
    Pc = BD.ref_dct2(BD.ref_dct2(c, mask), inverse=True)
    want = eps * Pc / Pc.flatten(1).norm(dim=1).reshape(n, 1, 1, 1)
    delta = ret["x_adv"] - x
    rel = (delta - want).flatten(1).norm(dim=1) / want.flatten(1).norm(dim=1)
    assert float(rel.max()) <= 1e-9, rel
    assert tuple(ret["norms"].shape) == (13, n) and float(ret["norms"].max()) <= eps * (1 + 1e-12)        # |w|_2 <= eps at every step
    assert float(ret["norms"][0].max()) == 0.0 and float(ret["norms"][-1].min()) >= eps * (1 - 1e-12)
    outside = BD.ref_dct2(delta, 1.0 - mask)
    assert float((outside * outside).sum()) <= 1e-12 and float(BD.ref_leak(ret["x_adv"], x, mask).max()) <= 1e-12
    assert bool((ret["coeff"] * (1.0 - mask) == 0).all())
    hist = ret["history"]
    assert torch.equal(hist[0], ret["loss0"]) and torch.equal(ret["best_loss"], hist.max(0).values) and bool((hist[1:] > hist[:-1])[:7].all())
    # targeted: the same point mirrored
    low = BD.ref_band_attack(fg, x, None, mask, eps, 12, step, targeted=True, clip=(-10.0, 10.0))
    assert float(((low["x_adv"] - x) + want).abs().max()) <= 1e-9 and bool((low["best_loss"] <= low["loss0"]).all())
    # an active clip is applied, and is what leaks
    cut = BD.ref_band_attack(fg, x, None, mask, eps, 3, step, clip=(-0.05, 0.05))
    assert float(cut["x_adv"].abs().max()) <= 0.05 and float(BD.ref_leak(cut["x_adv"], x, mask).max()) > 0


def _two_pass(w, G, step, eps):
    """step, then scale: the formulation the three dots replace"""
    n = w.shape[0]
    z = w + step * G / G.flatten(1).norm(dim=1).clamp_min(1e-12).reshape(n, 1)
    return z * (eps / z.flatten(1).norm(dim=1).clamp_min(1e-12)).clamp_max(1.0).reshape(n, 1)


def test_three_dot_identity():
    g = torch.Generator().manual_seed(5)
    w = torch.randn(6, 300, generator=g, dtype=torch.float64) * 0.05
    G = torch.randn(6, 300, generator=g, dtype=torch.float64)
    G[1] = 0.0                                                     # a uses the 1e-12 floor: no move
    w[2] = 0.0                                                     # from the origin
    w[3] = -0.25 * G[3] / G[3].norm() * (1 + 1e-16)                # the step lands (almost) on the origin: n2 cancels to ~0
    G[4] *= 1e-9
    G[5] *= 1e6
    for step, eps in ((0.25, 10.0), (0.25, 0.1), (-0.25, 0.1), (0.25, 0.0)):
        got, want = BD.ref_band_update(w, G, step, eps), _two_pass(w, G, step, eps)
        scale = want.abs().max(1).values.clamp_min(1e-3)
        assert float(((got - want).abs().max(1).values / scale).max()) <= 1e-12, (step, eps)
        assert float(got.norm(dim=1).max()) <= eps * (1 + 1e-12) or eps == 10.0
        if eps == 10.0:
            assert torch.equal(got[1], w[1])                        # G = 0 inside the ball: w stays as it is, to the bit
    # n2 slightly negative from cancellation: clamped at 0, never a NaN
    dots = torch.tensor([[1.0, -1.0 - 1e-16, 1.0]], dtype=torch.float64)
    out = BD.ref_band_update(torch.ones(1, 4, dtype=torch.float64) * 0.5, -torch.ones(1, 4, dtype=torch.float64) * 0.5, 1.0, 0.1,
                             dots=dots * torch.tensor([1.0, 1.0, 1.0]))
    assert bool(torch.isfinite(out).all())
    neg = torch.tensor([[1.0, -1.0000001, 1.0]], dtype=torch.float64)               # ww + 2 a wg + a^2 gg < 0 with a = 1
    assert float(1.0 + 2.0 * neg[0, 1] + 1.0) < 0
    out = BD.ref_band_update(torch.ones(1, 4, dtype=torch.float64), -torch.ones(1, 4, dtype=torch.float64), 1.0, 0.1, dots=neg)
    assert bool(torch.isfinite(out).all()) and bool((out == 0).all())               # w + a G is 0 here; s is finite


# ---- the parity bar rejects what it should ------------------------------------------------------------------------------------------------
def _dct_np(S, dtype, c0_as_cu=False, phase=1.0):
    i = np.arange(S, dtype=np.float64)
    D = np.sqrt(2.0 / S) * np.cos(np.pi * (2.0 * i[None, :] + phase) * i[:, None] / (2.0 * S))
    if not c0_as_cu:
        D[0] = np.sqrt(1.0 / S)
    return D.astype(dtype)


@pytest.mark.parametrize("S", [32, 95])
def test_parity_bar_rejects_subtly_wrong_transforms(S):
    rng = np.random.default_rng(S)
    x = rng.standard_normal((3, S, S)) + 0.75
    x[1] *= 1e3

    def rel(a, b):
        return float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max())

    D64, D32 = _dct_np(S, np.float64), _dct_np(S, np.float32)
    ref64 = D64 @ x @ D64.T
    yard = rel(D32 @ x.astype(np.float32) @ D32.T, ref64)
    bar, cause = bar_of(f"test_plane_dct2_vs_float64/ud_plane_dct2 S {S}", yard)
    assert cause is None and 2e-6 <= bar <= 1e-4 and yard < bar
    mutations = {"c_0 = c_u": (lambda D: D @ x @ D.T, _dct_np(S, np.float64, c0_as_cu=True)),
                 "phase 2i": (lambda D: D @ x @ D.T, _dct_np(S, np.float64, phase=0.0)),
                 "D^T X D": (lambda D: D.T @ x @ D, D64)}
    for name, (f, D) in mutations.items():
        e = rel(f(D), ref64)
        assert e >= 4.0 * bar, (name, e, bar)


# ---- refusals, resolution, the cache's key -------------------------------------------------------------------------------------------------
LOW = (0.0, 0.125)
BAD = [({"band": LOW, "norm": "linf"}, "norm must be one of ('l2',), got 'linf'"), ({"band": LOW}, "eps must be >= 0, got None"),
       ({"band": LOW, "eps": -1.0}, "eps must be >= 0"), ({"band": LOW, "eps": EPS, "steps": 0}, "steps must be an integer >= 1"),
       ({"band": LOW, "eps": EPS, "clip": (1.0, -1.0)}, "clip must be (lo, hi)"), ({"eps": EPS}, "exactly one of band=(lo, hi) and mask="),
       ({"band": LOW, "mask": torch.ones(64, 64), "eps": EPS}, "exactly one of band=(lo, hi) and mask="),
       ({"band": (0.5, 0.25), "eps": EPS}, "lo < hi"), ({"band": (-0.5, 0.25), "eps": EPS}, "lo must be a finite number >= 0"),
       ({"band": 0.5, "eps": EPS}, "band must be (lo, hi)"), ({"band": LOW, "shape": "ring", "eps": EPS}, "shape must be one of"),
       ({"mask": torch.ones(32, 32), "eps": EPS}, "mask must be a [64, 64] tensor"), ({"mask": [[1.0]], "eps": EPS}, "mask must be a [64, 64] tensor"),
       ({"band": LOW, "eps": EPS, "step": float("nan")}, "step must be a number"), ({"band": LOW, "eps": EPS, "objective": "margin"}, "objective must be"),
       ({"band": LOW, "eps": EPS, "precision": "bf16"}, "precision"), ({"band": LOW, "eps": EPS, "precision": "fp16"}, "fp16"),
       ({"band": LOW, "eps": EPS, "grad_scale": 3.0}, "grad_scale")]


@pytest.mark.parametrize("kw,text", BAD)
def test_refusals_need_no_device(kw, text):
    m = _model()
    for make in (lambda: BD.BandRunner(m, 2, 64, **kw), lambda: BD.band_runner(m, 2, 64, **kw), lambda: m.band_runner(2, 64, **kw)):
        with pytest.raises(ValueError, match=re.escape(text)):
            make()
    assert not m.__dict__.get("_ud_band_runners")


def test_host_side_refusals_and_resolution():
    from unidefense_amd.attack import resolve_step
    from unidefense_amd.model import load_model
    m = load_model("UDR18")(num_classes=2)
    with pytest.raises(ValueError, match="eval"):
        BD.BandRunner(m.train(), 2, 64, band=LOW, eps=EPS)
    with pytest.raises(ValueError, match="cuda"):                # every argument passed: only the device is missing
        BD.BandRunner(m.eval(), 2, 64, mask=torch.ones(64, 64), shape="square", eps=EPS, steps=3, step=0.1, targeted=True)
    with pytest.raises(ValueError, match="takes a UDEB4"):
        BD.BandRunner(torch.nn.Linear(2, 2), 2, 64, band=LOW, eps=EPS)
    with pytest.raises(ValueError, match="size must be <= 480"):
        BD.BandRunner(m.eval(), 2, 512, band=LOW, eps=EPS)
    for name in ("UDEB4", "UDR18", "UDR50"):
        assert callable(getattr(load_model(name), "band_runner"))
    a = BD._band_arguments(4, 128, band=LOW, eps=EPS)
    assert list(a) == ["batch", "size", "band", "shape", "mask", "eps", "steps", "step", "targeted", "clip", "objective", "precision",
                       "grad_scale", "norm"]
    assert (a["shape"], a["mask"], a["steps"], a["step"], a["targeted"], a["clip"], a["precision"], a["norm"]) == \
        ("radial", None, 10, None, False, (-1.0, 1.0), "fp32", "l2")
    assert a["objective"] is BD.cross_entropy_each and resolve_step(EPS, 10) == 0.25
    for call in (lambda: BD.dct2(torch.zeros(2, 8, 8)), lambda: BD.idct2(torch.zeros(2, 8, 8)),
                 lambda: BD.band_filter(torch.zeros(2, 8, 8), torch.ones(8, 8))):
        with pytest.raises(ValueError, match="cuda"):
            call()


def test_cache_key(monkeypatch):
    made = []

    class Stub:
        def __init__(self, model, *args):
            made.append(args)
            self.mask = None if args[4] is None else args[4].clone()          # as BandRunner: a copy the runner owns

        def set_mask(self, mask):
            self.mask.copy_(mask)

    monkeypatch.setattr(BD, "BandRunner", Stub)
    m = _model()
    r = BD.band_runner(m, 4, 128, band=LOW, eps=EPS)
    assert BD.band_runner(m, 4, 128, band=list(LOW), eps=EPS) is r and m.band_runner(4, 128, band=LOW, shape="radial", eps=EPS, steps=10) is r
    assert BD.band_runner(m, 4, 128, LOW, "radial", None, EPS, 10) is r and len(made) == 1
    held, other = torch.ones(128, 128), BD.band_mask(128, 0.25, 0.5)
    others = [BD.band_runner(m, 4, 128, eps=EPS, **kw) for kw in ({"band": (0.125, 0.25)}, {"band": LOW, "shape": "square"}, {"mask": held},
                                                                  {"band": LOW, "targeted": True}, {"band": LOW, "steps": 3})]
    assert len({id(o) for o in others + [r]}) == 6 and len(made) == 6
    # an explicit mask is contents, not a key: ONE runner per argument tuple, and every fetch copies the given mask into it
    by_mask = others[2]
    assert made[3][4] is held and by_mask.mask is not held and torch.equal(by_mask.mask, held) and made[1][2] == (0.125, 0.25)
    assert BD.band_runner(m, 4, 128, mask=other, eps=EPS) is by_mask and torch.equal(by_mask.mask, other) and len(made) == 6
    other.zero_()                                                                     # the caller's tensor is not aliased
    assert float(by_mask.mask.sum()) > 0
    # what a stage does, call after call: a fresh tensor each time, wherever the allocator puts it — always the one runner,
    # always reading the latest mask
    for k in range(8):
        fresh = torch.full((128, 128), float(k % 2))
        assert BD.band_runner(m, 4, 128, mask=fresh, eps=EPS) is by_mask and torch.equal(by_mask.mask, fresh)
        del fresh
    assert len(made) == 6 and BD.band_runner(m, 4, 128, mask=held, eps=EPS, steps=3) is not by_mask
    assert BD.band_key(4, 128, mask=held, eps=EPS) == BD.band_key(4, 128, mask=other, eps=EPS) != BD.band_key(4, 128, band=LOW, eps=EPS)
    assert BD.band_key(4, 128, band=LOW, eps=EPS) == BD.band_key(4, 128, band=list(LOW), eps=EPS, steps=10, norm="l2")
    assert BD.band_key(4, 128, band=LOW, eps=EPS) != BD.band_key(4, 128, band=LOW, eps=EPS, precision="fp16")
    assert BD.band_key(4, 128, band=LOW, eps=EPS, precision="fp16")[-2:] == ("fp16", 1024.0)
    from unidefense_amd.infer import _MAX_RUNNERS
    assert len(m.__dict__["_ud_band_runners"]) <= _MAX_RUNNERS
    assert not any(k.startswith("_ud_") and k != "_ud_band_runners" for k in m.__dict__)          # a dictionary of its own


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_refuse_bad_arguments():
    from tests.test_abi_cpu import header
    from unidefense_amd import kernels as K
    from unidefense_amd import lib
    h = header()
    L = ctypes.CDLL(lib.LIB_PATH)
    for n in ("ud_plane_dct2", "ud_band_dots", "ud_band_update"):
        assert n in h.protos and n in lib.EXPORTED and hasattr(L, n), n
        assert h.protos[n][0] is ctypes.c_int, n
        fn = getattr(L, n)
        fn.restype, fn.argtypes = ctypes.c_int, [t for t, _ in h.protos[n][1]]
    assert not any(n.startswith("ud_band") and n.endswith("_ws_bytes") for n in h.protos)     # the workspace is ud_sample_sumsq's, tripled
    for n in ("plane_dct2", "band_dots", "band_dots_ws_bytes", "band_update"):
        assert callable(getattr(K, n)), n
    buf = (ctypes.c_double * 64)()
    a, b, c, d, e, f = (ctypes.cast(ctypes.addressof(buf) + 64 * j, ctypes.c_void_p) for j in range(6))
    nan = float("nan")
    # (x, y, d, dt, mask, base, P, S, inverse, clip, lo, hi): mask and base may be NULL
    ok = (a, b, c, d, None, None, 3, 8, 0, 0, 0.0, 0.0, None)
    bad = [ok[:i] + (None,) + ok[i + 1:] for i in range(4)]
    bad += [(a, a) + ok[2:], (a, b, c, c) + ok[4:]]                                   # x == y, d == dt
    bad += [ok[:6] + t + (None,) for t in ((3, 1, 0, 0, 0.0, 0.0), (3, 0, 0, 0, 0.0, 0.0), (3, -8, 1, 0, 0.0, 0.0), (3, 481, 0, 0, 0.0, 0.0), (3, 496, 0, 0, 0.0, 0.0),
                                           (0, 8, 0, 0, 0.0, 0.0), (-3, 8, 1, 0, 0.0, 0.0), (1 << 31, 8, 0, 0, 0.0, 0.0),
                                           (3, 8, 1, 1, -1.0, 1.0), (3, 8, 0, 1, -1.0, 1.0))]   # clip without base
    with_base = (a, b, c, d, e, f)
    bad += [with_base + t + (None,) for t in ((3, 8, 1, 0, -1.0, 1.0),                # base without clip
                                              (3, 8, 0, 1, -1.0, 1.0),                # base on the forward transform
                                              (3, 8, 1, 1, 1.0, -1.0), (3, 8, 1, 1, nan, 1.0), (3, 8, 1, 1, -1.0, nan))]
    bad += [(a, b, c, d, e, b, 3, 8, 1, 1, -1.0, 1.0, None)]                          # base == y
    for args in bad:
        assert L.ud_plane_dct2(*args) == -1000, args
    # (w, g, N, per, out, ws, ws_bytes): ws may be NULL for one part
    ok = (a, b, 4, 12, c, None, 0, None)
    bad = [ok[:i] + (None,) + ok[i + 1:] for i in (0, 1, 4)]
    bad += [(a, b) + t + (c, None, 0, None) for t in ((0, 12), (-1, 12), (65536, 12), (4, 0), (4, -4), (4, 1 << 39))]
    bad += [(a, b, 4, 4097, c, None, 0, None), (a, b, 4, 4097, c, d, 8, None)]        # two parts: no ws, a ws too small
    for args in bad:
        assert L.ud_band_dots(*args) == -1000, args
    bad += [(a, b, 4, 4097, c, d, 4 * 2 * 3 * 8 - 1, None)]                           # one byte short of N parts 3 doubles
    for args in bad[-1:]:
        assert L.ud_band_dots(*args) == -1000, args
    assert K.band_dots_ws_bytes(4, 12) == 0 and K.band_dots_ws_bytes(4, 4096) == 0
    assert K.band_dots_ws_bytes(5, 4097) == 5 * 2 * 3 * 8 and K.band_dots_ws_bytes(2, 3 * 128 * 128) == 2 * 12 * 3 * 8
    # (w, g, dots, N, per, step, eps)
    ok = (a, b, c, 4, 12, 0.1, 0.1, None)
    bad = [ok[:i] + (None,) + ok[i + 1:] for i in range(3)] + [(a, a) + ok[2:]]
    bad += [ok[:3] + t + (None,) for t in ((0, 12, 0.1, 0.1), (65536, 12, 0.1, 0.1), (4, 0, 0.1, 0.1), (4, -2, 0.1, 0.1), (4, 12, nan, 0.1),
                                           (4, 12, 0.1, -0.1), (4, 12, 0.1, nan))]
    for args in bad:
        assert L.ud_band_update(*args) == -1000, args


def test_wrappers_refuse_cpu_tensors():
    from unidefense_amd import kernels as K
    x, D = torch.zeros(2, 3, 8, 8), torch.zeros(8, 8)
    for call in (lambda: K.plane_dct2(x, D, D.clone()), lambda: K.band_dots(x, x.clone()),
                 lambda: K.band_update(x, x.clone(), torch.zeros(2, 3, dtype=torch.float64), 0.1, 0.1)):
        with pytest.raises(ValueError, match="CUDA"):
            call()


# ---- the stage against stubs ---------------------------------------------------------------------------------------------------------------
DEV = torch.device("cpu")


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


def shift(mask):
    """the stub's perturbation: channel 0 moves by the share of the plane its mask covers"""
    return 0.5 * float(mask.mean())


class StubRunner:
    def __init__(self, net, mask, kwargs):
        self.net, self.mask = net, mask.clone()                      # as BandRunner: a copy the runner owns
        self.args = dict({"method": "band", "norm": "l2", "band": None, "clip": (-1.0, 1.0)}, **kwargs)
        self.leak = torch.zeros(4, dtype=torch.float64)

    def set_mask(self, mask):
        self.mask.copy_(mask)
        return self

    def __call__(self, x, y):
        self.net.log.append(("attack", float(self.mask.sum())))
        xa = x.clone()
        xa[:, 0] += shift(self.mask)
        self.leak = torch.full((x.shape[0],), 1.0 - float(self.mask.mean()), dtype=torch.float64)
        return xa.clamp(-1, 1)


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.log, self.runner = [], None

    def forward(self, x):
        self.log.append("forward")
        return {"cls_out": logits(x)}

    def band_runner(self, n, size, mask=None, shape="radial", eps=None, steps=10, clip=(-1.0, 1.0), precision="fp32"):
        self.log.append(("band_runner", n, size))
        if eps is None:
            raise ValueError("eps must be >= 0, got None")
        if self.runner is None:                                      # cached, as the model's accessor: the mask is refilled
            self.runner = StubRunner(self, mask, {"shape": shape, "eps": eps, "steps": steps, "precision": precision})
        return self.runner.set_mask(mask)


def removed(x, mask, clip):
    """the host stand-in of band_filter: channel 1 scaled by the share that is kept"""
    out = x.clone()
    out[:, 1] *= float(mask.mean())
    return out.clamp(*clip)


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


@pytest.mark.parametrize("bands", [None, [(0.0, 0.25), (0.25, None)]])
def test_stage_order_keys_control_and_removed_rows(bands, monkeypatch):
    gathered = []
    real = metrics.gather_scores
    monkeypatch.setattr(metrics, "gather_scores", lambda s, lb: gathered.append(s) or real(s, lb))
    ev, net, it = make()
    given = {"eps": 0.5, "steps": 3, "shape": "square"}
    if bands is not None:
        given["bands"] = bands
    before = dict(given)
    got = ev.test_band(2, given, band_filter=removed)
    assert given == before                                           # the caller's dict is not consumed
    assert it.steps == [1, 2]
    used = [tuple(b) for b in (bands or BD.DEFAULT_BANDS)]
    masks = [BD.band_mask(8, lo, hi, "square") for lo, hi in used]
    ones = torch.ones(8, 8)
    # ONE runner, asked for before any batch; per batch: clean, the control's attack and score, then per band attack, score, removed
    per_batch = ["forward", ("attack", 64.0), "forward"]
    for m in masks:
        per_batch += [("attack", float(m.sum())), "forward", "forward"]
    assert net.log == [("band_runner", 4, 8)] + per_batch * 2
    x, y = Batches.of([1, 2])

    def attacked(m):
        xa = x.clone()
        xa[:, 0] += shift(m)
        return p0(xa.clamp(-1, 1))

    assert set(got) == {"clean", "control", "bands", "attack"}
    same(got["clean"], expected(p0(x), y))
    right = (p0(x) < 0.5).long() == y
    assert 0 < int(right.sum()) < 8

    def check_row(row, m):
        same(row["adv"], expected(attacked(m), y))
        flipped = ((attacked(m) < 0.5).long() != y) & right
        assert type(row["fooled"]) is float and row["fooled"] == float(flipped.sum()) / float(right.sum())
        assert row["leak"] == pytest.approx(1.0 - float(m.mean()), abs=1e-15)

    assert set(got["control"]) == {"adv", "fooled", "leak"}
    check_row(got["control"], ones)                                  # the control row: the full spectrum
    assert got["control"]["leak"] == 0.0
    assert len(got["bands"]) == len(used)
    for row, b, m in zip(got["bands"], used, masks):
        assert set(row) == {"adv", "fooled", "leak", "band", "removed"} and row["band"] == b
        check_row(row, m)
        same(row["removed"], expected(p0(removed(x, 1.0 - m, (-1.0, 1.0))), y))       # the band removed, nothing attacked
    # the gathers, in order: clean, the control's adv and leak, then per band adv, leak, removed
    assert len(gathered) == 1 + 2 + 3 * len(used)
    assert torch.equal(gathered[0], p0(x)) and torch.equal(gathered[1], attacked(ones)) and torch.equal(gathered[3], attacked(masks[0]))
    assert torch.equal(gathered[5], p0(removed(x, 1.0 - masks[0], (-1.0, 1.0))))
    a = got["attack"]
    assert a["method"] == "band" and a["eps"] == 0.5 and a["steps"] == 3 and a["shape"] == "square" and a["bands"] == used
    assert got["control"]["fooled"] >= max(r["fooled"] for r in got["bands"])          # the stub moves most with the full mask


def test_stage_twice_on_one_model_attacks_inside_each_band_again():
    """the runner outlives the call: a second call must refill the mask the runner reads, not a tensor of its own"""
    ev, net, it = make()
    bands = [(0.0, 0.25), (0.25, None)]
    first = ev.test_band(1, {"eps": 0.5, "bands": bands}, band_filter=removed)
    runner = net.runner
    second = ev.test_band(1, {"eps": 0.5, "bands": bands}, band_filter=removed)
    assert net.runner is runner and net.log.count(("band_runner", 4, 8)) == 2
    for res in (first, second):
        for row in res["bands"]:
            assert not torch.equal(row["adv"]["scores"], res["control"]["adv"]["scores"]) and row["leak"] > res["control"]["leak"] == 0.0
    for a, b in zip(first["bands"] + [first["control"]], second["bands"] + [second["control"]]):
        assert torch.equal(a["adv"]["scores"], b["adv"]["scores"]) and a["leak"] == b["leak"]
    attacks = [e for e in net.log if isinstance(e, tuple) and e[0] == "attack"]
    assert attacks[:3] == attacks[3:] and len({a[1] for a in attacks[:3]}) == 3


def test_stage_passes_precision_and_refuses_before_any_batch():
    ev, net, it = make()
    ev.test_band(1, {"eps": 0.5, "precision": "fp16", "bands": [(0.0, None)]}, band_filter=removed)
    assert net.runner.args["precision"] == "fp16"
    ev, net, it = make()
    bad = (({"eps": 0.5, "epz": 0.1}, "^band takes BandRunner's keyword arguments and 'bands': .*epz"),
           ({"eps": 0.5, "band": (0.0, 0.5)}, "the stage sets 'band' itself"), ({"eps": 0.5, "mask": torch.ones(8, 8)}, "the stage sets 'mask' itself"),
           ({"eps": 0.5, "bands": [(0.5, 0.25)]}, "lo < hi"), ({"eps": 0.5, "bands": [(0.0, 0.5, 1.0)]}, "bands must be a list of"),
           ({"eps": 0.5, "bands": []}, "bands must be a list of"), ({"eps": 0.5, "bands": [0.5]}, "bands must be a list of"), ({"eps": 0.5, "shape": "ring"}, "shape must be one of"), ({}, "eps must be >= 0"),
           (None, "eps must be >= 0"))
    for band, text in bad:
        with pytest.raises(ValueError, match=text):
            ev.test_band(1, band, band_filter=removed)
    for batches in (0, 1.5):
        with pytest.raises(ValueError, match="batches must be an integer >= 1"):
            ev.test_band(batches, {"eps": 0.5}, band_filter=removed)
    assert it.steps == [] and "forward" not in net.log
    # the real accessor's refusals are ValueErrors already: they pass through, before any batch
    ev = evaluate.Evaluator(_model(), _model(), it, 2, 8, DEV)
    with pytest.raises(ValueError, match="eps must be >= 0"):
        ev.test_band(1, None)
    with pytest.raises(ValueError, match="band takes BandRunner's keyword arguments and 'bands'"):
        ev.test_band(1, {"eps": 0.1, "random_start": True})
    assert it.steps == []
    assert list(evaluate.ROBUST) == ["pgd", "apgd", "square", "apgd+square", "fmn", "sparse_fmn"]      # the stage is no ROBUST method
