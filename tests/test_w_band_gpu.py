"""GPU: the frequency-band attack's kernels (csrc/band.hip), BandRunner (unidefense_amd/band.py) and TrainEngine.test_band.

Kernels: the transform against the float64 restatement under the yardstick bar (tests/parity.py), its mask, base and clip
epilogues bitwise; the three dots against float64 numpy under ud_sample_sumsq's bar; the update against the restatement applied
to the GPU's own dots.  Runner: the life cycle (eager, capture, replay), the budget, the band (exact zeros outside it), the
keep-best rule, the leak against a float64 recomputation, what it leaves alone, and its EFFECT judged by the float64 oracle."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import param_fill
from tests.margins import within
from tests.parity import FLOOR, MARGIN, rel_err, yard_check
from tests.test_j_attack_gpu import _build, _dev, _loss64, _mixed_flags, _oracle_fwd, _rel_l2, _shared
from tests.test_r_universal_gpu import _bits, _place
from unidefense_amd import band as BD

pytestmark = pytest.mark.gpu

LO, HI = -1.0, 1.0
SHAPES = [(1, 2), (3, 4), (7, 20), (3, 32), (2, 36), (3, 95), (6, 128)]     # below one MFMA tile, one, a tail, odd, several strips
LARGE = [(2, 380), (1, 480)]        # the model's side that is no multiple of 32, and the largest side: 63360 bytes of LDS


def _planes_case(P, S, seed=0):
    """planes with a nonzero mean, one of them scaled by 1e3"""
    g = torch.Generator().manual_seed(1000 * S + P + seed)
    x = torch.randn(P, S, S, generator=g) + 0.75
    x[P // 2] *= 1e3
    return x


def _mask_case(S, seed=0):
    g = torch.Generator().manual_seed(77 + S + seed)
    m = (torch.rand(S, S, generator=g) < 0.5).float()
    m[0, 0], m[-1, -1] = 1.0, 0.0
    return m


def _chain32(x, mask=None, inverse=False):
    """the same chain in CPU float32: the yardstick"""
    D = BD.dct_matrix(x.shape[-1]).float()
    if inverse:
        return D.t() @ (x if mask is None else x * mask) @ D
    y = D @ x @ D.t()
    return y if mask is None else y * mask


def _mats(S, dev, offset=0):
    D = BD.dct_matrix(S)
    return _place(D.float().contiguous(), dev, offset), _place(D.t().contiguous().float(), dev, offset)


# ---- ud_plane_dct2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("P,S", SHAPES + LARGE)
def test_plane_dct2_vs_float64(P, S, offset):
    from unidefense_amd import kernels as K
    dev = _dev()
    x, mask = _planes_case(P, S), _mask_case(S)
    d, dt = _mats(S, dev, offset)
    xd, md = _place(x, dev, offset), _place(mask, dev, offset)
    before = xd.clone()
    for inverse in (False, True):
        for m, mdev in ((None, None), (mask, md)):
            out = _place(torch.zeros_like(x), dev, offset)
            got = K.plane_dct2(xd, d, dt, mdev, inverse=inverse, out=out)
            again = K.plane_dct2(xd, d, dt, mdev, inverse=inverse)
            torch.cuda.synchronize()
            assert np.array_equal(_bits(got), _bits(again))                              # a second launch: the same bits
            name = f"ud_plane_dct2 P {P} S {S} inverse {inverse} mask {m is not None} offset {offset}"
            ref64, ref32 = BD.ref_dct2(x, m, inverse), _chain32(x, m, inverse)
            yard_check(name, got, ref64, ref32)
            for p in range(P):                                        # and plane by plane: the scaled plane does not hide the others
                yard_check(f"{name} plane {p}", got[p], ref64[p], ref32[p])
    assert np.array_equal(_bits(xd), _bits(before))                                      # x is only read


@pytest.mark.parametrize("P,S", SHAPES)
def test_plane_dct2_masks_round_trip_and_public_functions(P, S):
    from unidefense_amd import kernels as K
    dev = _dev()
    x, mask = _planes_case(P, S, 1), _mask_case(S, 1)
    xd, md = x.to(dev), mask.to(dev)
    d, dt = _mats(S, dev)
    plain = K.plane_dct2(xd, d, dt, None)
    assert np.array_equal(_bits(plain), _bits(K.plane_dct2(xd, d, dt, torch.ones_like(md))))     # NULL mask: a mask of ones, bitwise
    masked = K.plane_dct2(xd, d, dt, md)
    out = (md == 0).expand(P, S, S)
    assert bool((masked[out] == 0).all()) and np.array_equal(_bits(masked[~out]), _bits(plain[~out]))
    assert np.array_equal(_bits(BD.dct2(xd)), _bits(plain)) and np.array_equal(_bits(BD.dct2(xd, mask)), _bits(masked))
    # idct2(dct2(x)) is x: the bar is the chain's own yardstick
    back = BD.idct2(BD.dct2(xd))
    yard_check(f"idct2(dct2(x)) P {P} S {S}", back, x.double(), _chain32(_chain32(x), inverse=True))
    assert np.array_equal(_bits(BD.band_project(xd, mask)), _bits(K.plane_dct2(masked, d, dt, None, inverse=True)))
    assert np.array_equal(_bits(BD.band_filter(xd, mask, (-2.0, 3.0))), _bits(BD.band_project(xd, mask).clamp(-2.0, 3.0)))
    # the inverse's epilogue: clamp(base + inverse, lo, hi) of its own no-base result, bitwise
    base = (torch.rand(P, S, S, generator=torch.Generator().manual_seed(S)) * 2 - 1).to(dev)
    coeff = masked * 1e-3
    inv = K.plane_dct2(coeff, d, dt, md, inverse=True)
    got = K.plane_dct2(coeff, d, dt, md, inverse=True, base=base, clip=(LO, HI))
    want = torch.clamp(base + inv, LO, HI)
    assert np.array_equal(_bits(got), _bits(want))
    assert bool((want == LO).any() | (want == HI).any()) or S < 4                        # the clip is active somewhere


def test_plane_dct2_keeps_a_nan_in_its_plane_and_wrappers_refuse():
    from unidefense_amd import kernels as K
    dev = _dev()
    P, S = 3, 36
    x = _planes_case(P, S, 2)
    x[1, 5, 7] = float("nan")
    d, dt = _mats(S, dev)
    for inverse in (False, True):
        got = K.plane_dct2(x.to(dev), d, dt, None, inverse=inverse)
        assert bool(torch.isnan(got[1]).all()) and not bool(torch.isnan(got[0]).any()) and not bool(torch.isnan(got[2]).any())
    xd = x.to(dev)
    with pytest.raises(Exception, match="status -1000"):                                 # x == y
        K.plane_dct2(xd, d, dt, None, out=xd)
    with pytest.raises(ValueError, match="base"):
        K.plane_dct2(xd, d, dt, None, inverse=True, base=xd.clone())
    with pytest.raises(ValueError, match="base"):
        K.plane_dct2(xd, d, dt, None, inverse=False, base=xd.clone(), clip=(LO, HI))
    with pytest.raises(ValueError, match="planes"):
        BD.dct2(torch.zeros(2, 8, 9, device=dev))
    with pytest.raises(ValueError, match="2 <= S <= 480"):
        BD.dct2(torch.zeros(1, 481, 481, device=dev))
    big = torch.zeros(1, 496, 496, device=dev)
    with pytest.raises(Exception, match="status -1000"):                                 # refused before any launch
        K.plane_dct2(big, *_mats(496, dev), None)
    with pytest.raises(ValueError, match="cuda"):
        BD.idct2(torch.zeros(2, 8, 8))


# ---- ud_band_dots / ud_band_update -----------------------------------------------------------------------------------------------------
ROWS = [(1, 1), (3, 75), (4, 192), (5, 4097), (33, 3072)]


def _rows_case(N, per, seed=0):
    """rows magnitudes apart"""
    g = torch.Generator().manual_seed(31 * N + per + seed)
    scale = (10.0 ** ((torch.arange(N) % 7) - 3.0)).reshape(N, 1)
    return torch.randn(N, per, generator=g) * scale, torch.randn(N, per, generator=g) * scale.flip(0)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("N,per", ROWS)
def test_band_dots_vs_float64(N, per, offset):
    """ud_sample_sumsq's bar (tests/test_j_attack_gpu.py): within per 2^-52 relative of numpy's float64 sum — terms added in
    double in another order.  For the signed dot <w, G> the same bound holds relative to the sum of the terms' magnitudes."""
    from unidefense_amd import kernels as K
    dev = _dev()
    w, g = _rows_case(N, per)
    wd, gd = _place(w, dev, offset), _place(g, dev, offset)
    got = K.band_dots(wd, gd)
    again = K.band_dots(wd, gd)
    torch.cuda.synchronize()
    assert got.dtype == torch.float64 and tuple(got.shape) == (N, 3) and torch.equal(got, again)
    w64, g64 = w.double().numpy(), g.double().numpy()
    want = np.stack([(w64 * w64).sum(1), (w64 * g64).sum(1), (g64 * g64).sum(1)], 1)
    size = np.stack([want[:, 0], np.abs(w64 * g64).sum(1), want[:, 2]], 1)
    rel = float((np.abs(got.cpu().numpy() - want) / size).max())
    assert within(f"ud_band_dots N {N} per {per} offset {offset}: |d| / sum|terms| / (per 2^-52)", rel / (per * 2.0 ** -52), 1.0)
    assert torch.equal(got[:, 0], K.sample_sumsq(wd))             # the same partition and tree as ud_sample_sumsq


@pytest.mark.parametrize("N,per", ROWS)
def test_band_update_vs_restatement(N, per):
    from unidefense_amd import kernels as K
    dev = _dev()
    w, g = _rows_case(N, per, 1)
    w = w * 0.1
    nrm = w.double().norm(dim=1)
    for step, eps in ((0.5, 10.0 * float(nrm.max()) + 1.0), (0.5, 0.25), (-0.25, 0.1 * float(nrm.min())), (0.3, 0.0)):
        wd, gd = w.clone().to(dev), g.to(dev)
        dots = K.band_dots(wd, gd)
        ref64 = BD.ref_band_update(w, g, step, eps, dots=dots.cpu())
        # the same chain in float32: the two factors from the double dots, as the kernel forms them, then fp32 arithmetic
        ww, wg, gg = dots.cpu().unbind(1)
        a = step / torch.sqrt(gg).clamp_min(1e-12)
        s = (eps / torch.sqrt((ww + 2.0 * a * wg + a * a * gg).clamp_min(0.0)).clamp_min(1e-12)).clamp_max(1.0)
        ref32 = s.float().reshape(-1, 1) * (w + a.float().reshape(-1, 1) * g)
        got = K.band_update(wd, gd, dots, step, eps)
        yard_check(f"ud_band_update N {N} per {per} step {step} eps {eps:.3g}", got, ref64, ref32)
        after = got.double().norm(dim=1).cpu()
        assert bool((after <= eps * (1 + 1e-6)).all()), (after, eps)
        assert bool(((s < 1.0) == (after >= eps * (1 - 1e-6)))[ref64.norm(dim=1) > 0].all())      # projected rows end on the sphere
        if 0.0 < eps < abs(step):
            assert bool((s < 1.0).any())                          # eps below the step: the projection is active
    # G = 0 inside the ball: a uses the 1e-12 floor, w stays as it is, bitwise
    wd = w.clone().to(dev)
    zero = torch.zeros_like(wd)
    K.band_update(wd, zero, K.band_dots(wd, zero), 0.5, float(nrm.max()) * 1.5)
    assert np.array_equal(_bits(wd), _bits(w))


# ---- the runner ------------------------------------------------------------------------------------------------------------------------
NAME, SIZE, N, STEPS, EPS = "UDEB4", 128, 2, 2, 1.0
LOW = BD.DEFAULT_BANDS[0]
KEYS = ("x_adv", "delta", "coeff", "best_loss", "loss0", "history", "norm", "leak")


def _inputs(seed, dev, scale=0.5):
    return (param_fill.make_input(N, SIZE, seed) * scale).to(dev), param_fill.make_labels(N).to(dev)


def _snapshot(r):
    return {k: getattr(r, k).detach().clone() for k in KEYS}


def _delta_bar(coeff, x):
    """(bar, float64 idct2(coeff)): the yardstick bar of the chain that makes x_adv - x with the clip inactive — the inverse
    transform of the coefficients, added to x and x taken off again — run in CPU float32 on the same coefficients"""
    w, xc = coeff.cpu(), x.cpu()
    ref64 = BD.ref_dct2(w, inverse=True)
    ref32 = (xc + _chain32(w.reshape(-1, *w.shape[-2:]), inverse=True).reshape(w.shape)) - xc
    return max(FLOOR, MARGIN * rel_err(ref32, ref64)), ref64


@functools.lru_cache(maxsize=None)
def _runs(precision, band):
    """eager, captured and two replayed calls of one runner on one input: shared by the tests that only read them"""
    dev = _dev()
    m = _shared(NAME, dev)
    x, y = _inputs(7, dev)
    r = BD.BandRunner(m, N, SIZE, band=band, eps=EPS, steps=STEPS, precision=precision)
    out = r(x, y)
    assert out is r.x_adv and r.graph is None
    eager = _snapshot(r)
    r(x, y)
    assert r.graph is not None and r.closing_graph is not None
    captured = _snapshot(r)
    r(x, y)
    return r, x, y, eager, captured, _snapshot(r)


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("band", [LOW, (0.25, 0.5), (0.0, None)])
def test_runner_life_cycle_and_structure(precision, band):
    r, x, y, eager, captured, replayed = _runs(precision, band)
    mask = BD.band_mask(SIZE, *band).to(x.device)
    for k in KEYS:                                                   # the replays are identical in bits
        assert np.array_equal(_bits(captured[k].float()), _bits(replayed[k].float())), k
    for k in ("x_adv", "coeff", "history"):
        rel = _rel_l2(replayed[k], eager[k])
        assert within(f"BandRunner {precision} {band}: replay vs eager warm-up {k}, rel L2", rel, 1e-5)
    for s in (eager, replayed):
        bar, delta64 = _delta_bar(s["coeff"], x)
        hist = s["history"]
        assert tuple(hist.shape) == (STEPS + 1, N) and bool(torch.isfinite(hist).all())
        assert torch.equal(hist[0], s["loss0"]) and bool((s["best_loss"] >= s["loss0"]).all())
        assert torch.equal(s["best_loss"], hist.max(0).values)      # the best of the steps + 1 visited points
        assert s["norm"].dtype == torch.float64 and bool((s["norm"] <= EPS * (1 + 1e-6)).all())
        assert float((s["norm"] - s["coeff"].double().flatten(1).norm(dim=1)).abs().max()) <= 1e-12
        outside = (mask == 0).expand(N, 3, SIZE, SIZE)
        assert not bool(s["coeff"][outside].any())                   # bitwise zero outside the band
        assert torch.equal(s["delta"], s["x_adv"] - x)
        # the clip is inactive (|x| <= 0.5, |delta| <= 1): x_adv - x is idct2(coeff) and nothing leaks out of the band
        assert float(s["x_adv"].abs().max()) < 1.0
        leak64 = BD.ref_leak(s["x_adv"].cpu(), x.cpu(), mask.cpu())
        print(f"  {precision} {band}: leak {s['leak'].tolist()}  float64 {leak64.tolist()}  bar^2 {bar * bar:.3e}")
        assert bool((s["leak"] <= bar * bar).all()) and bool((leak64 <= bar * bar).all())
        # ... and matches the float64 recomputation.  Both are rounding noise here, so they are compared as what they are: the
        # device forms sqrt(leak) |delta|_2 = |(1 - mask) dct2(delta)|_2 with an fp32 transform of delta, whose error is the
        # transform's bar times |delta|_2, so the two roots differ by at most that bar
        assert within(f"BandRunner {precision} {band}: |sqrt(leak) - sqrt(leak64)| / transform bar",
                      float((s["leak"].cpu().sqrt() - leak64.sqrt()).abs().max()) / bar, 1.0)
        assert within(f"BandRunner {precision} {band}: x_adv - x vs float64 idct2(coeff), max-norm rel", rel_err(s["delta"], delta64), bar)
    moved = replayed["best_loss"] > replayed["loss0"]
    assert bool(moved.any()), "no sample gained anything: the case shows nothing"
    assert bool((replayed["norm"][moved] > 0).all()) and not bool(replayed["coeff"][~moved].any())
    assert r.args["method"] == "band" and r.args["band"] == (band[0], band[1]) and r.args["step"] == 2.5 * EPS / STEPS
    assert all(p.grad is None for p in r.model.parameters()) and not r.model.training


def test_runner_follows_a_second_input_and_mask_equals_band():
    dev = _dev()
    r, x, y, _, _, replayed = _runs("fp32", LOW)
    x2, y2 = _inputs(8, dev)
    r(x2, y2)
    other = _snapshot(r)
    assert not torch.equal(other["history"], replayed["history"])
    m = _shared(NAME, dev)
    held = BD.band_mask(SIZE, *LOW).to(dev)
    by_mask = BD.BandRunner(m, N, SIZE, mask=held, eps=EPS, steps=STEPS)
    by_mask(x2, y2)
    got = _snapshot(by_mask)
    for k in ("x_adv", "coeff", "history"):                        # an eager first call against a replay
        assert within(f"BandRunner mask= vs band=: {k}, rel L2", _rel_l2(got[k], other[k]), 1e-5)
    assert by_mask.mask.data_ptr() != held.data_ptr() and torch.equal(by_mask.mask, held)      # the runner owns a copy ...
    held.zero_()
    assert torch.equal(by_mask.mask, BD.band_mask(SIZE, *LOW).to(dev))
    held = BD.band_mask(SIZE, 0.25, 0.5).to(dev)
    by_mask.set_mask(held.cpu().double())                            # ... and set_mask refills it: one runner, every band
    assert torch.equal(by_mask.mask, held)
    by_mask(x2, y2)
    by_mask(x2, y2)
    want = _runs("fp32", (0.25, 0.5))[0]
    outside = (held == 0).expand(N, 3, SIZE, SIZE)
    assert not bool(by_mask.coeff[outside].any()) and bool(by_mask.coeff.any())
    want(x2, y2)
    assert within("BandRunner refilled mask vs a runner of that band: x_adv, rel L2", _rel_l2(by_mask.x_adv, want.x_adv), 1e-5)
    assert m.band_runner(N, SIZE, band=LOW, eps=EPS, steps=STEPS) is m.band_runner(N, SIZE, band=list(LOW), eps=EPS, steps=STEPS)
    cached = m.band_runner(N, SIZE, mask=held, eps=EPS, steps=STEPS)                 # an explicit mask: one runner, refilled per fetch
    again = m.band_runner(N, SIZE, mask=torch.ones(SIZE, SIZE), eps=EPS, steps=STEPS)
    assert again is cached and bool((cached.mask == 1).all()) and cached.mask.data_ptr() != held.data_ptr()


def test_runner_leak_on_the_clip_bounds():
    """x pushed onto the clip bounds: the clamp cuts the perturbation, and what it cuts is not band-limited"""
    dev = _dev()
    m = _shared(NAME, dev)
    x, y = _inputs(9, dev, scale=1.0)
    x = torch.sign(x) * (1.0 - 1e-3 * x.abs())                       # within 1e-3 of -1 or 1
    mask = BD.band_mask(SIZE, *LOW)
    r = BD.BandRunner(m, N, SIZE, band=LOW, eps=4.0, steps=STEPS)
    for _ in range(3):
        r(x, y)
    leak64 = BD.ref_leak(r.x_adv.cpu(), x.cpu(), mask)
    print(f"  leak on the bounds {r.leak.tolist()}  float64 {leak64.tolist()}")
    moved = r.best_loss > r.loss0
    assert bool(moved.any()) and bool((r.leak[moved] > 0).all())
    rel = float(((r.leak.cpu() - leak64).abs() / leak64.clamp_min(1e-300))[moved.cpu()].max())
    assert within("BandRunner leak on the clip bounds vs float64, max rel", rel, 1e-4)
    assert float(r.x_adv.min()) >= LO and float(r.x_adv.max()) <= HI
    assert bool((r.norm <= 4.0 * (1 + 1e-6)).all())


@pytest.mark.parametrize("band", [LOW, (0.0, None)])
def test_runner_effect_judged_by_the_oracle(band):
    """the criterion of tests/test_j_attack_gpu.py: the oracle's loss at the GPU's x_adv against the same attack run in the oracle"""
    r, x, y, _, _, replayed = _runs("fp32", band)
    xc, yc = x.cpu(), y.cpu()
    mask = BD.band_mask(SIZE, *band)

    def forward_and_grad(xa, yy):
        xg = xa.detach().clone().requires_grad_()
        f = F.cross_entropy(_oracle_fwd(NAME, xg)["cls_out"], yy, reduction="none")
        g, = torch.autograd.grad(f.sum(), xg)
        return f.detach(), g

    ref = BD.ref_band_attack(forward_and_grad, xc, yc, mask, EPS, STEPS, r.step)
    with torch.no_grad():                                           # the oracle's own run has scored x and its x_adv already
        base, gain_ref = float(ref["loss0"].sum()), float(ref["best_loss"].sum() - ref["loss0"].sum())
        gain_gpu = float(_loss64(NAME, replayed["x_adv"].cpu().double(), yc)) - base
    ratio = gain_gpu / gain_ref
    print(f"  band {band}: L64(x) {base:.6g}  gain_ref {gain_ref:.4g}  gain_gpu {gain_gpu:.4g}  ratio {ratio:.5f}")
    assert gain_ref > 0
    assert float(ref["norms"].max()) <= EPS * (1 + 1e-12)
    assert within(f"band attack effect {band}: 1 - gain_gpu / gain_ref", 1.0 - ratio, 0.01)
    assert within(f"band attack {band}: history[0] vs the oracle's per-sample loss, max rel",
                  float(((replayed["loss0"].cpu().double() - ref["loss0"]).abs() / ref["loss0"]).max()), 1e-3)


def test_runner_leaves_the_model_alone_and_refuses():
    dev = _dev()
    m = _build(NAME, dev).eval()
    flags = _mixed_flags(m)
    bufs = {k: v.clone() for k, v in m.named_buffers()}
    x, y = _inputs(11, dev)
    r = BD.BandRunner(m, N, SIZE, band=(0.125, 0.25), shape="square", eps=EPS, steps=STEPS, targeted=True)
    for _ in range(3):
        r(x, y)
    assert bool((r.best_loss <= r.loss0).all()) and torch.equal(r.best_loss, r.history.min(0).values)      # targeted: descending
    assert [p.requires_grad for p in m.parameters()] == flags and all(p.grad is None for p in m.parameters()) and not m.training
    now = dict(m.named_buffers())
    assert all(torch.equal(v, now[k]) for k, v in bufs.items())
    with pytest.raises(ValueError, match="differs from the runner's key"):
        r(x[:1], y[:1])
    with pytest.raises(ValueError, match="differs from the runner's key"):
        r(x[:, :, :64, :64].contiguous(), y)
    with pytest.raises(ValueError, match="differ from the runner's key"):
        r(x, y.int())
    with pytest.raises(ValueError, match="cuda"):
        r(x.cpu(), y.cpu())
    m.train()
    with pytest.raises(ValueError, match="training mode"):
        r(x, y)
    with pytest.raises(ValueError, match="eval"):
        BD.BandRunner(m, N, SIZE, band=LOW, eps=EPS)
    m.eval()
    with pytest.raises(ValueError, match=r"mask must be a \[128, 128\] tensor"):
        BD.BandRunner(m, N, SIZE, mask=torch.ones(64, 64, device=dev), eps=EPS)


# ---- TrainEngine.test_band -------------------------------------------------------------------------------------------------------------
def test_engine_test_band():
    _dev()
    from tests.test_d_train_engine import CONFIG
    from tests.test_q_spatial_gpu import _same_result
    from unidefense_amd.engine import get_engine
    torch.manual_seed(0)
    eng = get_engine("FE")(copy.deepcopy(CONFIG), "Test")
    param_fill.fill_module_(eng.model_without_ddp, sf_coef=0.0, fuse_coef=0.3)       # weights whose input gradient is not zero
    t0 = eng.test(1)
    with pytest.raises(ValueError, match="band takes BandRunner's keyword arguments and 'bands'"):
        eng.test_band(batches=1, band={"eps": 1.0, "stepz": 3})
    with pytest.raises(ValueError, match="eps must be >= 0"):
        eng.test_band(batches=1, band={})
    bands = [(0.0, 0.25), (0.25, None)]
    res = eng.test_band(batches=1, band={"eps": 1.0, "steps": 2, "bands": bands})
    assert set(res) == {"clean", "control", "bands", "attack"}
    _same_result(res["clean"], t0)
    assert len(res["bands"]) == len(bands) and [b["band"] for b in res["bands"]] == bands
    assert set(res["control"]) == {"adv", "fooled", "leak"}
    for row in [res["control"]] + res["bands"]:
        assert set(row["adv"]) == set(t0) and torch.equal(row["adv"]["labels"], t0["labels"])
        assert 0.0 <= row["fooled"] <= 1.0 and 0.0 <= row["leak"] < 1.0
    for row in res["bands"]:
        assert set(row) == {"adv", "fooled", "leak", "band", "removed"} and set(row["removed"]) == set(t0)
    a = res["attack"]
    assert a["method"] == "band" and a["norm"] == "l2" and a["eps"] == 1.0 and a["steps"] == 2 and a["bands"] == bands
    assert all(p.grad is None for p in eng.model_without_ddp.parameters())
    # a second call on the same model: the ONE cached runner again, and it attacks inside each band again — the band rows differ
    # from the control row and repeat the first call's
    runners = eng.model_without_ddp.__dict__["_ud_band_runners"]
    assert len(runners) == 1
    runner = next(iter(runners.values()))
    res2 = eng.test_band(batches=1, band={"eps": 1.0, "steps": 2, "bands": bands})
    assert len(runners) == 1 and next(iter(runners.values())) is runner
    assert torch.equal(runner.mask, BD.band_mask(runner.size, *bands[-1]).to(runner.mask.device))      # the last band attacked
    for r in (res, res2):
        assert r["control"]["leak"] == 0.0 and not torch.equal(r["control"]["adv"]["scores"], r["clean"]["scores"])
        for row in r["bands"]:
            assert not torch.equal(row["adv"]["scores"], r["control"]["adv"]["scores"]) and row["leak"] > 0.0
            assert not torch.equal(row["removed"]["scores"], r["clean"]["scores"])
    assert not torch.equal(res["bands"][0]["adv"]["scores"], res["bands"][1]["adv"]["scores"])
    for a, b in zip(res["bands"] + [res["control"]], res2["bands"] + [res2["control"]]):
        assert within("test_band twice: adv scores of the second call vs the first, max |d|",
                      float((a["adv"]["scores"].double() - b["adv"]["scores"].double()).abs().max()), 1e-5)
