"""GPU: the flow-field attack's kernels (csrc/flow.hip), FlowRunner (unidefense_amd/flow.py) and TrainEngine.test_flow.

Kernels: the warp and the flow gradient against the float64 restatements with bars counted from the header's operation order,
the update bitwise against the torch fp32 expression and against ud_flow_warp, the control exactly against a Python loop.
Runner: the life cycle (eager, capture, replay), the bound (exact), the keep-best rule on its own history, what it leaves alone,
and its EFFECT judged by the float64 oracle."""
import copy
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import param_fill
from tests.margins import within
from tests.test_flow_cpu import make_flow, make_images
from tests.test_j_attack_gpu import _build, _dev, _grad64, _mixed_flags, _oracle_fwd, _rel_l2, _shared
from tests.test_r_universal_gpu import _bits
from unidefense_amd import flow as FL

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
# The bars count fp32 roundings on the longest path of the operation order the header states, times 2.
# ud_flow_warp: 1 - fx, its product with a tap, the sum of the two products, the product with 1 - fy, the last sum: 5 -> k = 10.
# Every intermediate is a convex combination of taps (|.| <= max|x|) or a weight in [0, 1], so each rounding adds at most
# 2^-24 max|x|; fx and fy themselves are exact (floor and px - x0 are exact in fp32, and the restatement starts from the same
# fp32 coordinate).
K_WARP = 10
# ud_flow_grad: the data term u01 - u00, its product with 1 - fy (itself one rounding, in parallel), the sum with the other
# product, the product with g, two channel adds: 6, every intermediate bounded by sum_ch |g| 2 max|x|.  The smoothness term:
# d = w(p) - w(q), d d, the sum of squares, + tv_eps, the root, the quotient (6, |quotient| <= 1), four adds (10), tau t (11).
# The last difference: 12 -> k = 24 on a magnitude of sum_ch |g| 2 max|x| + 4 tau.
K_GRAD = 24
SIZES = [2, 5, 33, 64, 130]                                        # below a tile, a tile's edge (64 columns, 4 rows), a tail
KINDS = ("zero", "integer", "small", "large", "bound", "half", "garbage")


def _flow(kind, n, S, seed):
    """the CPU suite's flow kinds, plus a small flow with NaN, +-inf and 1e30 entries"""
    if kind != "garbage":
        return make_flow(kind, n, S, seed)
    w = make_flow("small", n, S, seed)
    flat = w.view(-1)
    for i, v in enumerate((float("nan"), float("inf"), -float("inf"), 1e30, -1e30)):
        flat[(i * 7 + 1) % flat.numel()::max(flat.numel() // 3, 1) + 5 + i] = v
    return w


def _tame(w):
    """[N, S, S] bool: the pixel and its four neighbours hold finite, moderate displacements"""
    ok = (torch.isfinite(w) & (w.abs() < 1e3)).all(1)
    out = ok.clone()
    out[:, :, 1:] &= ok[:, :, :-1]
    out[:, :, :-1] &= ok[:, :, 1:]
    out[:, 1:, :] &= ok[:, :-1, :]
    out[:, :-1, :] &= ok[:, 1:, :]
    return out


def _same_nan(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b))


# ---- 1. ud_flow_warp ------------------------------------------------------------------------------------------------------------------
def _check_warp(n, S, kind, seed):
    dev = _dev()
    x, w = make_images(n, S, seed), _flow(kind, n, S, seed + 1)
    got = FL.flow_warp(x.to(dev), w.to(dev))
    torch.cuda.synchronize()
    got = got.cpu()
    want = FL.ref_flow_warp(x, w)
    assert _same_nan(got, want), (n, S, kind)
    fin = ~torch.isnan(want)
    worst = float(((got.double() - want)[fin].abs().max()) / (K_WARP * U24 * float(x.abs().max())))
    assert within(f"ud_flow_warp N {n} S {S} {kind}: |d| / ({K_WARP} 2^-24 max|x|)", worst, 1.0)
    if kind == "zero":
        assert np.array_equal(_bits(got), _bits(x))                  # bit for bit
    if kind == "garbage":                                           # NaN at the NaN pixels only; everything else finite
        bad = torch.isnan(w).any(1, keepdim=True).expand_as(got)
        assert bool(bad.any()) and torch.equal(torch.isnan(got), bad) and bool(torch.isfinite(got[~bad]).all())
    return got


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("n", [1, 3])
def test_warp_vs_float64(n, S):
    for i, kind in enumerate(KINDS):
        _check_warp(n, S, kind, 10 * S + i)


def test_warp_at_380():
    dev = _dev()
    _check_warp(1, 380, "small", 380)
    x = make_images(1, 380, 1).to(dev)
    w = torch.zeros(1, 2, 380, 380, device=dev)
    w[:, 0], w[:, 1] = 3.0, -2.0                                   # a whole-pixel flow is an exact shift away from the border
    got = FL.flow_warp(x, w)
    assert torch.equal(got[:, :, 2:, :377], x[:, :, :378, 3:])
    out = torch.empty_like(x)
    assert FL.flow_warp(x, w, out=out) is out and torch.equal(out, got)
    with pytest.raises(ValueError, match="not x itself"):
        FL.flow_warp(x, w, out=x)
    with pytest.raises(ValueError, match="the flow must be"):
        FL.flow_warp(x, w[:, :1])


# ---- 2. ud_flow_grad ------------------------------------------------------------------------------------------------------------------
def _check_grad(n, S, kind, seed, sign, tau):
    from unidefense_amd import kernels as K
    dev = _dev()
    x, w, g = make_images(n, S, seed), _flow(kind, n, S, seed + 1), make_images(n, S, seed + 2) * 0.01
    gw = torch.full((n, 2, S, S), 9.0, device=dev)
    K.flow_grad(g.to(dev), x.to(dev), w.to(dev), gw, sign, tau, 1e-8)
    torch.cuda.synchronize()
    got = gw.cpu().double()
    want = sign * FL.ref_flow_grad(g, x, w) - tau * FL.ref_flow_tv(w, 1e-8)[1]
    bar = K_GRAD * U24 * (g.double().abs().sum(1, keepdim=True) * 2.0 * float(x.abs().max()) + 4.0 * tau)
    ok = _tame(w).unsqueeze(1).expand_as(got)
    assert bool(ok.any()) or kind == "garbage"                      # the smallest sizes keep no pixel away from the garbage
    assert bool(torch.isfinite(got[ok]).all())
    worst = float(((got - want).abs() / bar)[ok].max()) if bool(ok.any()) else 0.0
    assert within(f"ud_flow_grad N {n} S {S} {kind} sign {sign} tau {tau}: |d| / ({K_GRAD} 2^-24 (sum|g| 2 max|x| + 4 tau))", worst, 1.0)
    if kind == "zero" and tau == 0.0:                               # a coordinate on the border does not move the sample: strict
        assert not bool(got[:, 0, :, 0].any()) and not bool(got[:, 0, :, -1].any())
        assert not bool(got[:, 1, 0, :].any()) and not bool(got[:, 1, -1, :].any())
        assert S < 3 or bool(got[:, :, 1:-1, 1:-1].any())
    return got


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("n", [1, 3])
def test_grad_vs_float64(n, S):
    for i, kind in enumerate(KINDS):
        for sign, tau in ((1, 0.0), (-1, 0.05)) if i % 2 else ((-1, 0.0), (1, 0.05)):
            _check_grad(n, S, kind, 20 * S + i, sign, tau)
    pos, neg = _check_grad(n, S, "small", 7, 1, 0.0), _check_grad(n, S, "small", 7, -1, 0.0)
    assert torch.equal(pos, -neg)                                   # the sign is an exact factor


def test_grad_at_380():
    _check_grad(1, 380, "small", 381, 1, 0.05)


# ---- 3. ud_flow_update ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,S", [(n, S) for n in (1, 3) for S in SIZES] + [(1, 380)])
def test_update_bitwise(n, S):
    from unidefense_amd import kernels as K
    dev = _dev()
    bound, step = 2.0, 0.3
    x = make_images(n, S, S).to(dev)
    for i, kind in enumerate(("small", "bound", "zero")):
        w0 = make_flow(kind, n, S, S + i).clamp(-bound, bound)
        gw = make_images(n, S, S + 5)[:, :2].clone()
        gw.view(-1)[::7] = 0.0                                      # sign(0) = sign(-0) = 0
        gw.view(-1)[3::14] = -0.0
        for keep in ([1] * n, [0] * n, [j % 2 for j in range(n)]):
            keep_t = torch.tensor(keep, dtype=torch.int32)
            w, wb = w0.clone().to(dev), torch.full_like(w0, 7.0).to(dev)
            xa = torch.full_like(x, 9.0)
            K.flow_update(w, wb, gw.to(dev), keep_t.to(dev), x, xa, step, bound)
            torch.cuda.synchronize()
            want_w = torch.clamp(w0 + step * torch.sign(gw), -bound, bound)              # torch fp32 ops: one rounding each
            want_b = torch.where(keep_t.bool().view(-1, 1, 1, 1), w0, torch.full_like(w0, 7.0))
            assert np.array_equal(_bits(w), _bits(want_w)) and np.array_equal(_bits(wb), _bits(want_b)), (n, S, kind, keep)
            assert np.array_equal(_bits(xa), _bits(FL.flow_warp(x, w)))
            # closing: w untouched, the image of w_best (which takes w where kept)
            w_before, xa2 = w.clone(), torch.full_like(x, 9.0)
            K.flow_update(w, wb, None, keep_t.to(dev), x, xa2, step, bound, closing=True)
            torch.cuda.synchronize()
            want_b = torch.where(keep_t.bool().view(-1, 1, 1, 1).to(dev), w_before, wb)
            assert np.array_equal(_bits(w), _bits(w_before)) and np.array_equal(_bits(wb), _bits(want_b))
            assert np.array_equal(_bits(xa2), _bits(FL.flow_warp(x, wb)))
    # a NaN in gw becomes a NaN in w and in x_adv at that pixel only; bound 0 returns x
    bad = gw.clone()
    bad[0, 1, S // 2, S // 3] = float("nan")
    w, wb, xa = w0.clone().to(dev), torch.zeros_like(w0).to(dev), torch.empty_like(x)
    K.flow_update(w, wb, bad.to(dev), torch.ones(n, dtype=torch.int32, device=dev), x, xa, step, bound)
    assert int(torch.isnan(w).sum()) == 1 and bool(torch.isnan(w[0, 1, S // 2, S // 3]))
    assert int(torch.isnan(xa).sum()) == 3 and bool(torch.isnan(xa[0, :, S // 2, S // 3]).all())
    w = torch.zeros_like(w0).to(dev)
    K.flow_update(w, wb, gw.to(dev), torch.ones(n, dtype=torch.int32, device=dev), x, xa, step, 0.0)
    assert not bool(w.any()) and np.array_equal(_bits(xa), _bits(x))


# ---- 4. ud_flow_control ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 5, 70])
def test_control_exact(N):
    from unidefense_amd import kernels as K
    dev = _dev()
    steps = 4
    gen = torch.Generator().manual_seed(N)
    for maximise in (True, False):
        ist, fst, history = K.flow_state(N, steps, dev)
        assert K.FLOW_I == {"k": 0, "keep": 1} and tuple(ist.shape) == (2, N) and tuple(history.shape) == (steps + 1, N)
        best = [0.0] * N
        for k in range(steps + 2):                                   # one call too many: it writes KEEP = 0 and nothing else
            f = (torch.rand(N, generator=gen) * 4).round() / 2       # a coarse grid: ties happen
            if k == 0:
                f[0] = float("nan")                                  # a NaN at k = 0 is taken, then replaced by the first number
            if N > 2 and k == 2:
                f[2] = float("nan")                                  # a NaN later never wins
            before = (history.clone(), fst.clone())
            K.flow_control(f.to(dev), ist, fst, history, maximise=maximise)
            torch.cuda.synchronize()
            if k == steps + 1:
                assert np.array_equal(_bits(history), _bits(before[0])) and np.array_equal(_bits(fst), _bits(before[1]))
                assert ist.cpu().tolist() == [[steps + 1] * N, [0] * N]
                break
            keep = []
            for n in range(N):                                       # the rule, as a Python loop
                fn, b = float(f[n]), best[n]
                better = fn > b if maximise else fn < b
                kp = k == 0 or better or (math.isnan(b) and not math.isnan(fn))
                if kp:
                    best[n] = fn
                keep.append(int(kp))
            assert ist.cpu().tolist() == [[k + 1] * N, keep], (N, k, maximise)
            assert np.array_equal(_bits(history[k]), _bits(f))
            assert np.array_equal(_bits(fst[0]), _bits(torch.tensor(best, dtype=torch.float32)))
        assert keep is not None and not math.isnan(best[0])


# ---- 5. the runner ------------------------------------------------------------------------------------------------------------------
CASES = [("UDR18", 128, 2, 5, "fp32"), ("UDEB4", 256, 1, 7, "fp32"), ("UDEB4", 256, 1, 7, "fp16")]
STEPS = 3


def _inputs(size, n, seed, dev):
    return param_fill.make_input(n, size, seed).to(dev), param_fill.make_labels(n).to(dev)


def _snapshot(r):
    torch.cuda.synchronize()
    return {k: getattr(r, k).clone() for k in ("x_adv", "flow", "best_loss", "loss0", "history", "flow_linf", "flow_tv")}


@functools.lru_cache(maxsize=None)
def _oracle_each(name, size, n, seed):
    x, y = param_fill.make_input(n, size, seed).double(), param_fill.make_labels(n)
    with torch.no_grad():
        return F.cross_entropy(_oracle_fwd(name, x)["cls_out"], y, reduction="none")


@pytest.mark.parametrize("name,size,n,seed,precision", CASES)
def test_life_cycle_bound_and_keep_best(name, size, n, seed, precision):
    dev = _dev()
    m = _shared(name, dev)
    x, y = _inputs(size, n, seed, dev)
    r = FL.FlowRunner(m, n, size, max_flow=2.0, steps=STEPS, step=0.75, tau=0.05, precision=precision)
    assert r.args["method"] == "flow" and r.args["step"] == 0.75 and r.args["max_flow"] == 2.0
    xa = r(x, y)
    assert r.graph is None and r.calls == 1 and xa is r.x_adv and not xa.requires_grad
    eager = _snapshot(r)
    r(x, y)
    assert r.graph is not None and r.closing_graph is not None
    captured = _snapshot(r)
    r(x, y)
    replayed = _snapshot(r)
    for k in captured:                                              # the replays are identical in bits
        assert np.array_equal(_bits(captured[k]), _bits(replayed[k])), k
    for k in ("x_adv", "history"):
        rel = _rel_l2(replayed[k], eager[k])
        print(f"  {name} {precision}: replay vs eager {k}, rel L2 {rel:.3e}")
        assert within(f"FlowRunner {name} {precision}: replay vs eager warm-up {k}, rel L2", rel, 1e-5)
    for s in (eager, replayed):
        flow, hist = s["flow"], s["history"]
        assert tuple(flow.shape) == (n, 2, size, size) and tuple(hist.shape) == (STEPS + 1, n)
        assert float(flow.abs().max()) <= 2.0 and bool(torch.isfinite(hist).all())      # the bound, exact
        assert np.array_equal(_bits(s["x_adv"]), _bits(FL.flow_warp(x, flow)))
        assert torch.equal(s["best_loss"], hist.max(0).values) and torch.equal(s["loss0"], hist[0])
        assert bool((s["best_loss"] >= s["loss0"]).all())
        first = hist.argmax(0)                                       # torch returns the first maximum: ties keep the earliest
        assert bool((hist.gather(0, first.view(1, -1))[0] == s["best_loss"]).all())
        assert torch.equal(s["flow_linf"], flow.abs().flatten(1).amax(1))
        tv = FL.ref_flow_tv(flow.cpu(), 1e-8)[0]
        assert within(f"FlowRunner {name} {precision}: flow_tv vs float64, max rel", ((s["flow_tv"].cpu().double() - tv).abs() / tv).max(), 1e-5)
    # the winning flow is one of the points visited: a sample that improved holds a flow with a component at a multiple of the step
    moved = replayed["best_loss"] > replayed["loss0"]
    assert bool(moved.any()), "no sample gained anything: the case shows nothing"
    assert bool((replayed["flow_linf"][moved] >= 0.75).all()) and not bool(replayed["flow"][~moved].any())
    each = _oracle_each(name, size, n, seed)
    rel = float(((replayed["loss0"].cpu().double() - each).abs() / each).max())
    print(f"  {name} {precision}: history[0] vs the oracle's per-sample loss, max rel {rel:.3e}")
    assert within(f"FlowRunner {name} {precision}: history[0] vs the oracle's per-sample loss, max rel", rel, 1e-3)
    # a second input is followed on replay
    x2, y2 = _inputs(size, n, seed + 1, dev)
    r(x2, y2)
    other = _snapshot(r)
    assert not torch.equal(other["history"], replayed["history"])
    assert np.array_equal(_bits(other["x_adv"]), _bits(FL.flow_warp(x2, other["flow"])))
    fresh = FL.FlowRunner(m, n, size, max_flow=2.0, steps=STEPS, step=0.75, tau=0.05, precision=precision)
    fresh(x2, y2)
    assert within(f"FlowRunner {name} {precision}: replay on a second input vs a fresh eager run, history rel L2",
                  _rel_l2(other["history"], fresh.history), 1e-5)
    assert all(p.grad is None for p in m.parameters()) and not m.training


def test_targeted_descends_and_zero_bound_returns_the_input():
    dev = _dev()
    m = _shared("UDR18", dev)
    x, y = _inputs(128, 2, 5, dev)
    r = FL.FlowRunner(m, 2, 128, max_flow=2.0, steps=STEPS, step=0.75, targeted=True)
    for _ in range(3):
        r(x, y)
        torch.cuda.synchronize()
        assert torch.equal(r.best_loss, r.history.min(0).values) and bool((r.best_loss <= r.loss0).all())
        assert bool((r.best_loss < r.loss0).any())
    z = FL.FlowRunner(m, 2, 128, max_flow=0.0, steps=2)
    assert z.step == 0.0
    for _ in range(3):
        assert np.array_equal(_bits(z(x, y)), _bits(x)) and not bool(z.flow.any()) and not bool(z.flow_linf.any())
    with pytest.raises(ValueError, match="differs from the runner's key"):
        z(x[:1], y[:1])


def test_runner_leaves_the_model_as_it_was():
    dev = _dev()
    m = _build("UDR18", dev).eval()
    flags = _mixed_flags(m)
    assert not all(flags) and any(flags)
    bufs = {k: v.clone() for k, v in m.named_buffers()}
    params = [p.detach().clone() for p in m.parameters()]
    x, y = _inputs(128, 2, 5, dev)
    r = FL.FlowRunner(m, 2, 128, steps=2)
    for _ in range(3):
        r(x, y)
    torch.cuda.synchronize()
    assert [p.requires_grad for p in m.parameters()] == flags and all(p.grad is None for p in m.parameters()) and not m.training
    now = dict(m.named_buffers())
    assert all(torch.equal(v, now[k]) for k, v in bufs.items())
    assert all(torch.equal(a, b) for a, b in zip(params, m.parameters()))
    assert m.flow_runner(2, 128, steps=2) is m.flow_runner(2, 128, steps=2)


# ---- 6. effect, judged by the oracle -----------------------------------------------------------------------------------------------
EFFECT = ("UDR18", 128, 2, 5)
EFFECT_KW = dict(max_flow=0.25, steps=STEPS, step=0.125, tau=0.05, tv_eps=1e-8)      # every w a dyadic number: exact in fp32


def oracle_flow(name, size, n, seed, noise=0.0, noise_seed=0, max_flow=2.0, steps=STEPS, step=0.75, tau=0.05, tv_eps=1e-8):
    """FlowRunner's algorithm run wholly in float64 on the oracle's gradients with the ref_* functions: (the clean summed loss,
    the best flow, its gain).  noise: uniform noise of that fraction of max|g| added to every gradient (the bar's simulation)."""
    x, y = param_fill.make_input(n, size, seed).double(), param_fill.make_labels(n)
    gen = torch.Generator().manual_seed(noise_seed)

    def each(xa):
        with torch.no_grad():
            return F.cross_entropy(_oracle_fwd(name, xa)["cls_out"], y, reduction="none")

    w = torch.zeros(n, 2, size, size, dtype=torch.float64)
    w_best, best = w.clone(), torch.zeros(n, dtype=torch.float64)
    for k in range(steps + 1):
        xa = FL.ref_flow_warp(x, w)
        keep, best = FL.ref_flow_control(each(xa), k, best, True)
        if k == steps:
            w_best = torch.where(keep.view(-1, 1, 1, 1), w, w_best)
            break
        g = _grad64(name, xa, y)
        if noise:
            g = g + (torch.rand(g.shape, generator=gen, dtype=torch.float64) * 2 - 1) * noise * float(g.abs().max())
        gw = FL.ref_flow_grad(g, x, w) - tau * FL.ref_flow_tv(w, tv_eps)[1]
        w, w_best = FL.ref_flow_update(w, w_best, gw, keep, step, max_flow)
    base = float(each(x).sum())
    return base, w_best, float(each(FL.ref_flow_warp(x, w_best)).sum()) - base


# The bar on 1 - gain_gpu / gain_ref: re-running oracle_flow on the CPU with uniform noise of 1e-4 max|g| in its gradient moved
# the gain by 5.1e-3 and 5.4e-3 of itself on this case (gain_ref 4.6622 on a loss of 2.7719; ratios 0.99491, 1.00543 for the noise
# seeds 1, 2): below 1e-2, so the suite's 0.1 (test_attack_effect_judged_by_the_oracle) stands.  The settings were chosen on the
# CPU before any GPU run: at max_flow 0.25 the random +-max_flow control LOSES 0.38 (control / gain_ref -0.082); at max_flow 2.0 a
# random flow scrambles the image enough to gain 0.745 of what the attack gains in three steps, and the same noise moves the gain
# by 5-9 %, so that budget shows little about the gradient (profiles/r25/flow.txt).
EFFECT_BAR = 0.1


def test_effect_judged_by_the_oracle():
    name, size, n, seed = EFFECT
    dev = _dev()
    m = _shared(name, dev)
    x, y = param_fill.make_input(n, size, seed), param_fill.make_labels(n)
    r = FL.FlowRunner(m, n, size, **EFFECT_KW)
    r(x.to(dev), y.to(dev))
    r(x.to(dev), y.to(dev))
    torch.cuda.synchronize()
    flow = r.flow.cpu()
    base, ref, gain_ref = oracle_flow(name, size, n, seed, **EFFECT_KW)

    def loss(w):
        with torch.no_grad():
            return float(F.cross_entropy(_oracle_fwd(name, FL.ref_flow_warp(x, w))["cls_out"], y, reduction="sum"))

    gain_gpu = loss(flow) - base
    control = (torch.randint(0, 2, (n, 2, size, size), generator=torch.Generator().manual_seed(0)).float() * 2 - 1) * EFFECT_KW["max_flow"]
    gain_control = loss(control) - base
    ratio = gain_gpu / gain_ref
    agree = float((flow.double() == ref).double().mean())
    print(f"  {name}: L64(x) {base:.6g}  gain_ref {gain_ref:.4g}  gain_gpu {gain_gpu:.4g}  ratio {ratio:.5f}  control {gain_control:.4g}  "
          f"share of flow components equal to the oracle's {agree:.4f}")
    assert gain_ref > 0
    assert within(f"flow effect {name}: 1 - gain_gpu / gain_ref", 1.0 - ratio, EFFECT_BAR)
    assert within(f"flow effect {name}: the random +-max_flow control's gain / gain_ref", gain_control / gain_ref, 0.1)


# ---- 7. the stage ---------------------------------------------------------------------------------------------------------------------
def test_engine_test_flow():
    _dev()
    from tests.test_d_train_engine import CONFIG
    from tests.test_q_spatial_gpu import _same_result
    from unidefense_amd.engine import get_engine
    torch.manual_seed(0)
    eng = get_engine("FE")(copy.deepcopy(CONFIG), "Test")
    t0 = eng.test(1)
    with pytest.raises(ValueError, match="flow takes FlowRunner's keyword arguments"):
        eng.test_flow(batches=1, flow={"max_flow": 1.0, "stepz": 3})
    res = eng.test_flow(batches=1, flow={"max_flow": 1.0, "steps": 2})
    assert set(res) == {"clean", "adv", "attack"}
    _same_result(res["clean"], t0)
    assert set(res["adv"]) == set(t0) and torch.equal(res["adv"]["labels"], t0["labels"])
    a = res["attack"]
    assert {"method", "max_flow", "steps", "step", "tau", "tv_eps", "targeted", "objective", "precision", "grad_scale", "flow_linf_mean",
            "flow_linf_max", "flow_tv_mean", "flow_tv_max", "fooled"} == set(a)
    assert a["method"] == "flow" and a["max_flow"] == 1.0 and a["steps"] == 2 and a["step"] == 2.5 * 1.0 / 2
    assert 0.0 <= a["flow_linf_mean"] <= a["flow_linf_max"] <= 1.0 and 0.0 < a["flow_tv_mean"] <= a["flow_tv_max"]
    assert 0.0 <= a["fooled"] <= 1.0                               # half of this fixture's samples are classified correctly clean
    assert all(p.grad is None for p in eng.model_without_ddp.parameters())
