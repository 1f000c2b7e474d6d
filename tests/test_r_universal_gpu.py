"""GPU: the universal perturbation's kernels (csrc/universal.hip), UniversalRunner (unidefense_amd/universal.py) and
TrainEngine.test_universal.

Kernels: the batch reduction bitwise against a numpy float32 loop, the L-infinity update and the apply bitwise against the
torch fp32 expression, the L2 chain against the float64 restatement with the bars of tests/test_j_attack_gpu.py's
test_l2_step_and_projection_vs_float64, the control exactly.  Runner: the life cycle (eager, capture, replay), the pattern's
persistence across calls (exact), its budget (exact), what it leaves alone, the clamped-loss rule on known losses, the reduce
hook, and its EFFECT judged by the float64 oracle."""
import copy
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import param_fill
from tests.margins import within
from tests.test_j_attack_gpu import _build, _dev, _grad64, _loss64, _mixed_flags, _oracle_fwd, _rel_l2, _shared
from unidefense_amd import universal as U

pytestmark = pytest.mark.gpu

LO, HI = -1.0, 1.0
EPS4 = 4.0 / 255.0
EPS4_F32 = float(torch.tensor(EPS4))                             # the budget as the kernels hold it: delta is fp32
SHAPES = [(1, 1), (3, 75), (4, 192), (5, 4097), (33, 3072)]     # scalar path, vector path, a tail, more samples than a wave's quarter
OFFSET = (4, 192, True)                                          # a vector shape from a base one float off 16 bytes: scalar path
KERNEL_CASES = [s + (False,) for s in SHAPES] + [OFFSET]


def _place(t, dev, offset):
    """t on the device; offset: inside a larger buffer, one float behind a 16-byte boundary"""
    if not offset:
        return t.to(dev).contiguous()
    big = torch.zeros(t.numel() + 1, dtype=t.dtype, device=dev)
    out = big[1:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


# ---- 1. ud_uap_reduce: bitwise ---------------------------------------------------------------------------------------------------
def _np_reduce(g, w):
    """the float32 loop: ascending n from 0.f, one add per counted term"""
    g = g.numpy()
    acc = np.zeros(g.shape[1], dtype=np.float32)
    for n in range(g.shape[0]):
        if int(w[n]) != 0:
            acc = (acc + g[n]).astype(np.float32)
    return acc


@pytest.mark.parametrize("N,per,offset", KERNEL_CASES)
def test_reduce_bitwise_vs_float32_loop(N, per, offset):
    from unidefense_amd import kernels as K
    dev = _dev()
    gen = torch.Generator().manual_seed(N * 31 + per)
    g = torch.randn(N, per, generator=gen) * torch.logspace(-3, 3, N).reshape(N, 1)      # magnitudes apart: the order of adds shows
    g[:, ::9] = 0.0
    gd = _place(g, dev, offset)
    some = (torch.arange(N) % 3 != 1).to(torch.int32)                                     # zeros among the weights
    some[0] = 1
    for w in (some, torch.ones(N, dtype=torch.int32), torch.zeros(N, dtype=torch.int32), 7 * some):
        got = K.uap_reduce(gd, w.to(dev), _place(torch.full((per,), 9.0), dev, offset))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(got), _np_reduce(g, w).view(np.uint32)), (N, per, w.tolist())
    assert not bool(K.uap_reduce(gd, torch.zeros(N, dtype=torch.int32, device=dev), torch.ones(per, device=dev)).any())
    # a NaN in an excluded row stays out; in a counted row it shows, at its element only
    e = per // 2
    if N >= 2:
        bad = g.clone()
        bad[1, e] = float("nan")
        got = K.uap_reduce(_place(bad, dev, offset), some.to(dev), torch.empty(per, device=dev))
        assert int(some[1]) == 0 and np.array_equal(_bits(got), _np_reduce(g, some).view(np.uint32))
    bad = g.clone()
    bad[0, e] = float("nan")
    got = K.uap_reduce(_place(bad, dev, offset), some.to(dev), torch.empty(per, device=dev)).cpu()
    want = torch.from_numpy(_np_reduce(g, some))
    keep = torch.arange(per) != e
    assert bool(torch.isnan(got[e])) and np.array_equal(_bits(got[keep]), _bits(want[keep]))


# ---- 2. ud_uap_update_linf and ud_uap_apply: bitwise -------------------------------------------------------------------------------
def _pattern_case(N, per, seed):
    gen = torch.Generator().manual_seed(seed)
    delta = (torch.rand(per, generator=gen) * 2 - 1) * EPS4
    delta[1::5] = EPS4                               # on the budget's faces
    delta[2::5] = -EPS4
    gsum = torch.randn(per, generator=gen)
    gsum[::7] = 0.0                                  # exact zeros: sign(0) = 0
    gsum[5::14] = -0.0
    x = torch.rand(N, per, generator=gen) * 2 - 1
    x[:, 3::11] = LO                                 # on the clip bounds
    x[:, 4::13] = HI
    return delta, gsum, x


@pytest.mark.parametrize("N,per,offset", KERNEL_CASES)
def test_update_linf_and_apply_bitwise_vs_torch(N, per, offset):
    from unidefense_amd import kernels as K
    dev = _dev()
    delta, gsum, x = _pattern_case(N, per, N + per)
    xd = _place(x, dev, offset)
    for step, eps in ((EPS4 / 4, EPS4), (-EPS4 / 4, EPS4), (EPS4, EPS4), (EPS4 / 4, 0.0)):
        want_d = torch.clamp(delta + step * torch.sign(gsum), -eps, eps)                 # torch fp32 ops: one rounding each
        want_x = torch.clamp(x + want_d, LO, HI)
        d, xa = _place(delta, dev, offset), _place(torch.full_like(x, 9.0), dev, offset)
        K.uap_update_linf(d, _place(gsum, dev, offset), xd, xa, step, eps, LO, HI)
        torch.cuda.synchronize()
        assert torch.equal(d.cpu(), want_d) and torch.equal(xa.cpu(), want_x), (N, per, step, eps)
        if eps == 0.0:
            assert not bool(d.any()) and torch.equal(xa.cpu(), x.clamp(LO, HI))
    assert torch.equal(xd.cpu(), x)                                                      # x is only read
    # apply without a norm: delta is only read; any N; x_adv may be x
    d = _place(delta, dev, offset)
    xa = K.uap_apply(d, None, xd, _place(torch.full_like(x, 9.0), dev, offset), EPS4, LO, HI)
    assert torch.equal(xa.cpu(), torch.clamp(x + delta, LO, HI)) and torch.equal(d.cpu(), delta)
    one = K.uap_apply(d, None, xd[:1], torch.empty_like(xd[:1]), EPS4, LO, HI)
    assert torch.equal(one.cpu(), torch.clamp(x[:1] + delta, LO, HI))
    inplace = xd.clone()
    K.uap_apply(d, None, inplace, inplace, EPS4, LO, HI)
    assert torch.equal(inplace, xa)
    # a NaN in gsum stays visible in delta and in every sample's x_adv, there only
    bad = gsum.clone()
    bad[per // 2] = float("nan")
    d, xa = delta.clone().to(dev), torch.empty(N, per, device=dev)
    K.uap_update_linf(d, bad.to(dev), x.to(dev), xa, EPS4 / 4, EPS4, LO, HI)
    assert int(torch.isnan(d).sum()) == 1 and bool(torch.isnan(d[per // 2])) and int(torch.isnan(xa).sum()) == N


# ---- 3. the L2 chain against float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,per,offset", KERNEL_CASES)
def test_l2_chain_vs_float64(N, per, offset):
    """step and projection each against the float64 rule applied to the GPU's own input of that stage, with the bars of
    test_l2_step_and_projection_vs_float64 for the same helpers: 4 2^-24 (|value| + |change|)"""
    from unidefense_amd import kernels as K
    dev = _dev()
    delta, gsum, x = _pattern_case(N, per, 3 * N + per)
    nrm = float(delta.double().norm())

    def chain(d0, gs, step, eps):
        d, g1 = _place(d0, dev, offset).view(1, -1), _place(gs, dev, offset).view(1, -1)
        K.attack_step_l2(d, g1, K.sample_sumsq(g1), step)
        stepped = d.clone().cpu().view(-1)
        xa = K.uap_apply(d.view(-1), K.sample_sumsq(d), _place(x, dev, offset), torch.empty(N, per, device=dev), eps, LO, HI)
        torch.cuda.synchronize()
        return stepped, d.cpu().view(-1), xa.cpu()

    for step, eps in ((0.5 * nrm, 0.8 * nrm), (-0.25 * nrm, 0.8 * nrm), (0.1 * nrm, 4.0 * nrm)):
        stepped, got, xa = chain(delta, gsum, step, eps)
        inc = step * gsum.double() / max(float(gsum.double().norm()), 1e-12)
        want = U.ref_uap_update_l2(delta, gsum, step, math.inf)                          # the step alone
        bound = 4 * 2.0 ** -24 * (delta.double().abs() + inc.abs())
        worst = float(((stepped.double() - want).abs() / bound.clamp_min(1e-300)).max())
        assert within(f"uap L2 step N {N} per {per}: |d| / (4 2^-24 (|delta| + |increment|))", worst, 1.0)
        want = U.ref_uap_update_l2(stepped, torch.zeros(per), 0.0, eps)                  # the projection alone
        bound = 4 * 2.0 ** -24 * stepped.double().abs()
        worst = float(((got.double() - want).abs() / bound.clamp_min(1e-300)).max())
        assert within(f"uap L2 projection N {N} per {per}: |d| / (4 2^-24 |delta|)", worst, 1.0)
        if float(stepped.double().norm()) <= eps:
            assert torch.equal(got, stepped)                                             # a factor of exactly 1: untouched
        else:
            assert float(got.double().norm()) <= eps * (1 + 2.0 ** -23)                   # one relative 2^-24 rounding per element
        assert torch.equal(xa, torch.clamp(x + got, LO, HI))
    # no counted sample: gsum = 0 moves nothing (0 / max(0, 1e-12)), no NaN; eps = 0: the zero pattern
    stepped, got, xa = chain(delta, torch.zeros(per), 0.5 * nrm, 4.0 * nrm)
    assert torch.equal(stepped, delta) and torch.equal(got, delta)
    _, got, xa = chain(delta, gsum, 0.5 * nrm, 0.0)
    assert not bool(got.any()) and torch.equal(xa, x.clamp(LO, HI))


# ---- 4. ud_uap_control: exact -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 5, 70])
def test_control_exact(N):
    from unidefense_amd import kernels as K
    dev = _dev()
    steps = 3
    gen = torch.Generator().manual_seed(N)
    for beta, source in ((math.inf, None), (1.0, None), (math.inf, 0), (math.inf, 1), (1.0, 1)):
        ist, w, history, counted = K.uap_state(N, steps, dev)
        assert K.UAP_I == {"k": 0} and tuple(ist.shape) == (1, N)
        fs = []
        for k in range(steps + 1):                                   # one call too many: it writes nothing
            f = torch.rand(N, generator=gen) * 2.0
            f[0] = 1.0                                               # f == beta is not below it
            if N > 2:
                f[2] = float("nan")                                  # compares false: not counted
            y = torch.randint(0, 2, (N,), generator=gen)
            before = (history.clone(), counted.clone(), w.clone())
            K.uap_control(f.to(dev), y.to(dev), w, ist, history, counted, beta, source)
            torch.cuda.synchronize()
            if k == steps:
                assert np.array_equal(_bits(history), _bits(before[0])) and torch.equal(counted, before[1]) and torch.equal(w, before[2])
                assert ist.cpu().tolist() == [[steps] * N]
                break
            fs.append(f)
            want = U.ref_uap_control(f, y, beta, source).to(torch.int32)
            assert torch.equal(w.cpu(), want) and torch.equal(counted[k].cpu(), want) and ist.cpu().tolist() == [[k + 1] * N]
            assert int(want[0]) == (0 if beta == 1.0 else int(source is None or int(y[0]) == source))
            assert N <= 2 or int(want[2]) == 0
            assert np.array_equal(_bits(history[k]), _bits(f))
            if source is not None:
                assert not bool(want[y != source].any())
        assert np.array_equal(_bits(history), _bits(torch.stack(fs)))


# ---- 5. the runner ------------------------------------------------------------------------------------------------------------------
CASES = [("UDR18", 128, 4, 5, "fp32"), ("UDEB4", 256, 2, 7, "fp32"), ("UDEB4", 256, 2, 7, "fp16")]


def _inputs(size, n, seed, dev):
    return param_fill.make_input(n, size, seed).to(dev), param_fill.make_labels(n).to(dev)


def _fit(r, x, y, calls=1):
    """delta and x_adv after reset() and `calls` calls"""
    r.reset()
    for _ in range(calls):
        xa = r(x, y)
    torch.cuda.synchronize()
    return r.delta.clone(), xa.clone()


# the L2 chain differs from the L-infinity launch behind the backward only: one model carries it
@pytest.mark.parametrize("name,size,n,seed,precision,norm", [c + ("linf",) for c in CASES] + [CASES[0] + ("l2",)])
def test_life_cycle_persistence_and_budget(name, size, n, seed, precision, norm):
    dev = _dev()
    m = _shared(name, dev)
    x, y = _inputs(size, n, seed, dev)
    per = 3 * size * size
    eps = EPS4 if norm == "linf" else 1.0
    kw = dict(norm=norm, eps=eps, step=eps / 4, precision=precision)
    r2, r4 = U.UniversalRunner(m, n, size, steps=2, **kw), U.UniversalRunner(m, n, size, steps=4, **kw)
    assert tuple(r2.delta.shape) == (3, size, size) and not bool(r2.delta.any()) and r2.args["step"] == eps / 4
    # call 1 (eager) against calls 2 and 3 (capture, replay), each from a reset()
    eager, xa_eager = _fit(r2, x, y)
    assert r2.graph is None and r2.calls == 1
    d2, xa2 = _fit(r2, x, y)
    d3, xa3 = _fit(r2, x, y)
    assert r2.graph is not None and r2.update_graph is None and r2.calls == 3
    assert torch.equal(d2, d3) and torch.equal(xa2, xa3)
    rel = _rel_l2(d2, eager)
    print(f"  {name} {precision} {norm}: replay vs eager delta, rel L2 {rel:.3e}")
    assert within(f"UniversalRunner {name} {precision} {norm}: replay vs eager warm-up delta, rel L2", rel, 1e-5)
    # delta persists: two calls of two steps are one call of four steps from the same start, bit for bit
    twice, xa_twice = _fit(r2, x, y, calls=2)
    h_second = r2.history.clone()
    _fit(r4, x, y)
    once, xa_once = _fit(r4, x, y)
    assert r4.graph is not None
    assert torch.equal(twice, once) and torch.equal(xa_twice, xa_once) and not torch.equal(twice, d2)
    assert torch.equal(h_second, r4.history[2:]) and tuple(r4.history.shape) == (4, n) and tuple(r4.counted.shape) == (4, n)
    assert bool((r4.counted == 1).all()) and r4.counted.dtype == torch.int32             # beta = inf: everyone steers
    # the budget and the clip, exact
    for d, xa in ((eager, xa_eager), (d2, xa2), (once, xa_once)):
        assert torch.isfinite(d).all() and float(xa.min()) >= LO and float(xa.max()) <= HI
        assert torch.equal(xa, torch.clamp(x + d, LO, HI))
        if norm == "linf":
            assert float(d.abs().max()) <= EPS4_F32 and float(d.abs().max()) > 0.4 * eps
        else:
            nrm = float(d.double().norm())
            assert 0.2 * eps < nrm <= eps * (1 + 2.0 ** -23), nrm                      # one relative 2^-24 rounding per element
    # apply: any batch size, no backward, the runner's pattern as it stands
    other = param_fill.make_input(3, size, seed + 1).to(dev) * 1.02
    got = r4.apply(other)
    assert got.data_ptr() != other.data_ptr() and not got.requires_grad
    assert torch.equal(got, torch.clamp(other + once, LO, HI)) and torch.equal(r4.delta, once)
    out = torch.empty_like(other)
    assert r4.apply(other, out=out) is out and torch.equal(out, got)
    with pytest.raises(ValueError, match="cuda"):
        r4.apply(other.cpu())
    with pytest.raises(ValueError, match="batch"):
        r4.apply(other[:, :, :-1])
    assert all(p.grad is None for p in m.parameters()) and not m.training
    assert per == once.numel()


@pytest.mark.parametrize("norm", ["linf", "l2"])
def test_zero_budget_returns_the_clamped_input(norm):
    dev = _dev()
    m = _shared("UDR18", dev)
    x = (param_fill.make_input(4, 128, 5) * 1.02).to(dev)           # a few values outside clip
    y = param_fill.make_labels(4).to(dev)
    assert float(x.max()) > HI
    r = U.UniversalRunner(m, 4, 128, norm=norm, eps=0.0, steps=2)
    assert r.step == 0.0
    for _ in range(3):
        assert torch.equal(r(x, y), x.clamp(LO, HI)) and not bool(r.delta.any())


def test_runner_leaves_the_model_as_it_was():
    dev = _dev()
    m = _build("UDR18", dev).eval()
    flags = _mixed_flags(m)
    assert not all(flags) and any(flags)
    bufs = {k: v.clone() for k, v in m.named_buffers()}
    x, y = _inputs(128, 4, 5, dev)
    for r in (U.UniversalRunner(m, 4, 128, eps=EPS4, steps=2), U.UniversalRunner(m, 4, 128, norm="l2", eps=0.5, steps=2),
              U.UniversalRunner(m, 4, 128, eps=EPS4, reduce=lambda g: None)):
        for _ in range(3):
            r(x, y)
    torch.cuda.synchronize()
    assert [p.requires_grad for p in m.parameters()] == flags and all(p.grad is None for p in m.parameters()) and not m.training
    now = dict(m.named_buffers())
    assert all(torch.equal(v, now[k]) for k, v in bufs.items())


@functools.lru_cache(maxsize=None)
def _oracle(name, size, n, seed):
    """(per-sample clean losses, their sum, the pattern of four sign iterations at eps 4/255, step eps / 4, run wholly in the
    float64 oracle, its gain): computed once per case"""
    x = param_fill.make_input(n, size, seed).double()
    y = param_fill.make_labels(n)
    with torch.no_grad():
        each = F.cross_entropy(_oracle_fwd(name, x)["cls_out"], y, reduction="none")
    delta = torch.zeros(3, size, size, dtype=torch.float64)
    for _ in range(4):
        xa = U.ref_uap_apply(delta, x, LO, HI)
        g = _grad64(name, xa, y)                                    # the sum's gradient: each sample's own
        delta = U.ref_uap_update_linf(delta, U.ref_uap_reduce(g, torch.ones(n)), EPS4 / 4, EPS4)      # beta = inf: everyone steers
    with torch.no_grad():
        gain = float(_loss64(name, U.ref_uap_apply(delta, x, LO, HI), y)) - float(each.sum())
    return each, float(each.sum()), delta, gain


def test_clamped_loss_rule_on_known_losses():
    """the oracle's clean losses of the UDR18 case are 2.74, 3.48, 0.060 and 0.047: beta = 1.0 is far from all four"""
    dev = _dev()
    m = _shared("UDR18", dev)
    x, y = _inputs(128, 4, 5, dev)
    each = _oracle("UDR18", 128, 4, 5)[0]
    assert [round(float(v), 2 if v > 1 else 3) for v in each] == [2.74, 3.48, 0.060, 0.047]
    r = U.UniversalRunner(m, 4, 128, eps=EPS4, steps=1, beta=1.0)
    for _ in range(3):                                              # eager, captured, replayed
        _fit(r, x, y)
        assert r.counted.cpu().tolist() == [[0, 0, 1, 1]]
        rel = float(((r.history[0].cpu().double() - each).abs() / each).max())
        assert within("UniversalRunner UDR18 history[0] vs the oracle's per-sample loss, max rel", rel, 1e-3)
    # only samples 2 and 3 steered: the pattern is the sign of THEIR gradients' sum
    want = EPS4 / 10 * torch.sign(r.g[2] + r.g[3])
    assert torch.equal(r.delta, want) and r.args["beta"] == 1.0 and r.args["step"] == EPS4 / 10
    src = U.UniversalRunner(m, 4, 128, eps=EPS4, steps=1, source=1)
    _fit(src, x, y)
    assert src.counted.cpu().tolist() == [(y == 1).int().cpu().tolist()] and src.args["source"] == 1


def test_reduce_hook():
    dev = _dev()
    m = _shared("UDR18", dev)
    x, y = _inputs(128, 4, 5, dev)
    calls = []

    def zeroing(gsum):
        calls.append(tuple(gsum.shape))
        gsum.zero_()

    def identity(gsum):
        calls.append("identity")

    plain = U.UniversalRunner(m, 4, 128, eps=EPS4, steps=2, step=EPS4 / 4)
    _fit(plain, x, y)
    want, xa_want = _fit(plain, x, y)
    for norm, eps in (("linf", EPS4), ("l2", 1.0)):
        r = U.UniversalRunner(m, 4, 128, norm=norm, eps=eps, steps=2, reduce=zeroing)
        start = (torch.rand(3, 128, 128, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(dev) * (eps / 400)
        for call in range(3):                                       # eager, captured, replayed: two graphs with the hook between
            del calls[:]
            r.delta.copy_(start)
            xa = r(x, y)
            assert calls == [(3, 128, 128)] * 2 and torch.equal(r.delta, start), (norm, call)
            assert torch.equal(xa, torch.clamp(x + start, LO, HI))
        assert r.graph is not None and r.update_graph is not None
    r = U.UniversalRunner(m, 4, 128, eps=EPS4, steps=2, step=EPS4 / 4, reduce=identity)
    _fit(r, x, y)
    del calls[:]
    got, xa = _fit(r, x, y)
    assert calls == ["identity"] * 2 and torch.equal(got, want) and torch.equal(xa, xa_want)      # the bits of reduce=None


# ---- 6. effect, judged by the oracle -----------------------------------------------------------------------------------------------
# The bar on 1 - gain_gpu / gain_ref: re-running the oracle's four iterations with uniform noise of 1e-4 max|g| in its gradient
# (4 x the x.grad error DESIGN 3j records) moved the gain by <= 5e-4 of itself on the UDR18 case (gain_ref 6.4985 on a loss of
# 6.3248; ratios 0.99996, 1.00048): the suite's 0.1 (test_attack_effect_judged_by_the_oracle) stands there.  On the UDEB4 case the
# pattern gains little (gain_ref 8.61e-4 on a loss of 1.6014: the filled model is nearly flat at this budget) and the same noise
# loses 3.92e-2 and 3.90e-2 of it (ratios 0.96078, 0.96100) — more than 1e-2, so that case's bar is ten times the simulated loss.
EFFECT_BAR = {"UDR18": 0.1, "UDEB4": 0.392}


@pytest.mark.parametrize("name,size,n,seed,precision", CASES[:2])
def test_effect_judged_by_the_oracle(name, size, n, seed, precision):
    dev = _dev()
    m = _shared(name, dev)
    x = param_fill.make_input(n, size, seed)
    y = param_fill.make_labels(n)
    r = U.UniversalRunner(m, n, size, eps=EPS4, steps=4, step=EPS4 / 4, precision=precision)
    _fit(r, x.to(dev), y.to(dev))
    delta, _ = _fit(r, x.to(dev), y.to(dev))
    each, base, ref, gain_ref = _oracle(name, size, n, seed)
    sign = torch.randint(0, 2, (3, size, size), generator=torch.Generator().manual_seed(0)).double() * 2 - 1
    with torch.no_grad():
        gain_gpu = float(_loss64(name, U.ref_uap_apply(delta.cpu(), x, LO, HI), y)) - base
        gain_control = float(_loss64(name, U.ref_uap_apply(sign * EPS4, x, LO, HI), y)) - base
    ratio = gain_gpu / gain_ref
    agree = float((torch.sign(delta.cpu().double()) == torch.sign(ref)).double().mean())
    print(f"  {name} {precision}: L64(x) {base:.6g}  gain_ref {gain_ref:.4g}  gain_gpu {gain_gpu:.4g}  ratio {ratio:.5f}  "
          f"control {gain_control:.4g}  share of elements with the oracle's sign {agree:.4f}")
    assert gain_ref > 0
    assert within(f"universal effect {name} {precision}: 1 - gain_gpu / gain_ref", 1.0 - ratio, EFFECT_BAR[name])
    assert within(f"universal effect {name}: the random-sign control's gain / gain_ref", gain_control / gain_ref, 0.1)


# ---- 7. the stage ---------------------------------------------------------------------------------------------------------------------
def test_engine_test_universal():
    _dev()
    from tests.test_d_train_engine import CONFIG
    from unidefense_amd.engine import get_engine
    cfg = copy.deepcopy(CONFIG)
    cfg["model"] = {"name": "UDR18", "num_classes": 2, "drop_rate": 0.2}
    cfg["data"] = {"train_batch_size": 2, "size": 128}
    cfg["config"]["universal"] = {"norm": "linf", "eps": EPS4, "steps": 2, "seed": 1}
    eng = get_engine("FE")(cfg, "Test")
    param_fill.fill_module_(eng.model_without_ddp, sf_coef=0.0, fuse_coef=0.3)
    with pytest.raises(ValueError, match="universal takes UniversalRunner's keyword arguments and 'seed'"):
        eng.test_universal(batches=1, fit_batches=1, epochs=1, universal={"eps": EPS4, "stepz": 3})
    res = eng.test_universal(batches=1, fit_batches=1, epochs=1)
    assert set(res) == {"clean", "adv", "control", "attack"}
    a = res["attack"]
    assert {"method", "norm", "eps", "steps", "step", "beta", "source", "clip", "precision", "delta", "linf", "l2", "fooled",
            "fooled_control", "fit_counted"} <= set(a)
    assert a["method"] == "universal" and a["eps"] == EPS4 and a["steps"] == 2 and a["step"] == EPS4 / 10
    assert a["delta"].device.type == "cpu" and tuple(a["delta"].shape) == (3, 128, 128)
    assert 0 < a["linf"] <= EPS4_F32 and a["linf"] == float(a["delta"].abs().max()) and a["l2"] > 0
    assert a["fit_counted"] == [4, 4]
    for k in ("clean", "adv", "control"):
        assert tuple(res[k]["scores"].shape) == (4,) and torch.equal(res[k]["labels"], res["clean"]["labels"])
    assert not torch.equal(res["adv"]["scores"], res["clean"]["scores"])
    assert not torch.equal(res["control"]["scores"], res["adv"]["scores"])
    # the held-out step is the iterator's step 2: the clean column is test()'s second batch
    assert torch.equal(res["clean"]["scores"], eng.test(batches=2)["scores"][4:])
    assert all(p.grad is None for p in eng.model_without_ddp.parameters())
