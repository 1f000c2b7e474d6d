"""GPU: the sparse minimum-norm attack — the kernels of csrc/sfmn.hip and the graph-replayed SparseFMNRunner
(unidefense_amd/attack.py; TrainEngine.test_robust with "method": "sparse_fmn").

Kernels: ud_sfmn_norm_parts against float64 numpy (sums to 1e-12 relative, the maximum and the count exactly), ud_sfmn_control
step by step against the state machine of tests/test_sparse_fmn_cpu.py (every state array equal), ud_sfmn_select +
ud_sfmn_apply against the float64 projections there (l0: the kept set and every bit; l1: every element within 2^-22 max(1, |ref|)
of the reference rounded to fp32 and the ball held).  Runner: replay, clip, radius and found properties (exact), the objective at
x_adv against the forward, the EFFECT judged by the float64 oracle, and what the runner must leave alone.

As in tests/test_n_fmn_gpu.py the trajectories are printed, never asserted."""
import copy
import functools

import numpy as np
import pytest
import torch

from oracle import param_fill
from tests import oracle_util as ou
from tests.margins import within
from tests.test_j_attack_gpu import (_build, _mean_ce, _mixed_flags, _oracle_fwd, _rel_l2, _same_result, _shared, _train_grads)
from tests.test_n_fmn_gpu import _eb4_objective, _norm_case, _same, _view
from tests.test_sparse_fmn_cpu import (CHUNK, DABS, DCNT, GMAX, GSS, ONE_DECISION, ref_project_l0, ref_project_l1, ref_sfmn_control,
                                       ref_sfmn_norm_parts, ref_sfmn_worst, ref_sparse_fmn)

pytestmark = pytest.mark.gpu

LO, HI = -1.0, 1.0
INF = float("inf")
NAN = float("nan")
ALPHA = {"l1": 8.0, "l0": 256.0}             # the L2-normalised step sized to the norm (SparseFMNRunner's docstring)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    ou.fit_cpu_threads()
    return torch.device("cuda:0")


# ---- 1. ud_sfmn_norm_parts ---------------------------------------------------------------------------------------------------
def _folded(parts):
    p = np.asarray(parts, dtype=np.float64)
    return p[:, :, GSS].sum(1), p[:, :, GMAX].max(1), p[:, :, DABS].sum(1), p[:, :, DCNT].sum(1)


def _sparse_norm_case(N, per, seed, shift):
    """tests/test_n_fmn_gpu.py's case with every third element of x equal to x0, so that the count is not per"""
    fx, fx0, fg = _norm_case(N, per, seed, shift)
    fx[shift:shift + N * per:3] = fx0[shift:shift + N * per:3]
    return fx, fx0, fg


@pytest.mark.parametrize("N,per", [(1, 1), (3, 5), (1, 4096), (3, 4097), (3, 3 * 32 * 32)])
def test_norm_parts_vs_float64(N, per):
    """the sums within 1e-12 relative of numpy's float64 (<= 4096 non-negative terms per part in double either way), the maximum
    of |g| exactly, the count exactly (every part against the reference's part, not only the fold).  shift 1 takes the scalar
    path at every per; g = None leaves the g entries as they were."""
    from unidefense_amd import kernels as K
    dev = _dev()
    parts = (per + CHUNK - 1) // CHUNK
    assert K.sfmn_norms_ws_bytes(N, per) == N * parts * 32
    for shift in (0, 1):
        fx, fx0, fg = _sparse_norm_case(N, per, 13 * N + per + shift, shift)
        dx, dx0, dg = (_view(f.to(dev), N, per, shift) for f in (fx, fx0, fg))
        assert dx.data_ptr() % 16 == 4 * shift and dx.is_contiguous()
        ws = torch.full((N, parts, 4), -7.0, dtype=torch.float64, device=dev)
        K.sfmn_norm_parts(dx, dx0, dg, ws=ws)
        got = ws.cpu().numpy()
        want = ref_sfmn_norm_parts(*(_view(f, N, per, shift).numpy() for f in (fx, fx0, fg)))
        assert np.array_equal(got[:, :, DCNT], want[:, :, DCNT]) and np.array_equal(got[:, :, GMAX], want[:, :, GMAX])
        assert float(want[:, :, DCNT].sum()) == float((_view(fx, N, per, shift) != _view(fx0, N, per, shift)).sum())
        for name, j in (("sum g^2", GSS), ("sum |x - x0|", DABS)):
            g_, w_ = _folded(got)[(GSS, GMAX, DABS, DCNT).index(j)], _folded(want)[(GSS, GMAX, DABS, DCNT).index(j)]
            rel = float(np.max(np.abs(g_ - w_) / np.maximum(np.abs(w_), 1e-300)))
            assert within(f"ud_sfmn_norm_parts N {N} per {per} shift {shift}: {name} vs float64, max rel", rel, 1e-12)
        assert torch.equal(K.sfmn_norm_parts(dx, dx0, dg), ws)                      # the default workspace: the same bits
        ws2 = torch.full((N, parts, 4), -7.0, dtype=torch.float64, device=dev)
        K.sfmn_norm_parts(dx, dx0, None, ws=ws2)                                    # the closing form
        assert torch.equal(ws2[:, :, [DABS, DCNT]], ws[:, :, [DABS, DCNT]])
        assert bool((ws2[:, :, [GSS, GMAX]] == -7.0).all())


@pytest.mark.parametrize("N,per", [(3, 5), (3, 4097), (3, 3 * 32 * 32)])
def test_norm_parts_keeps_a_nan_in_its_own_entries(N, per):
    """a NaN in x shows in the sample's sum |x - x0| (and counts as one differing element) and nowhere else; a NaN in g shows in
    its two g entries only"""
    from unidefense_amd import kernels as K
    dev = _dev()
    fx, fx0, fg = _sparse_norm_case(N, per, per, 0)
    x, x0, g = (_view(f, N, per, 0).clone() for f in (fx, fx0, fg))
    clean = _folded(K.sfmn_norm_parts(x.to(dev), x0.to(dev), g.to(dev)).cpu().numpy())
    for at in sorted({0, per // 2, per - 1}):
        xb = x.clone()
        xb[1, at] = NAN
        got = _folded(K.sfmn_norm_parts(xb.to(dev), x0.to(dev), g.to(dev)).cpu().numpy())
        assert np.isnan(got[2][1]) and got[3][1] == clean[3][1] + (1.0 if float(x[1, at]) == float(x0[1, at]) else 0.0), at
        assert got[0][1] == clean[0][1] and got[1][1] == clean[1][1]
        for j in range(4):
            assert got[j][0] == clean[j][0] and got[j][2] == clean[j][2]
        gb = g.clone()
        gb[2, at] = NAN
        got = _folded(K.sfmn_norm_parts(x.to(dev), x0.to(dev), gb.to(dev)).cpu().numpy())
        assert np.isnan(got[0][2]) and np.isnan(got[1][2]) and got[2][2] == clean[2][2] and got[3][2] == clean[3][2], at
        for j in range(4):
            assert got[j][0] == clean[j][0] and got[j][1] == clean[j][1]


# ---- 2. ud_sfmn_control: every state array, step by step ---------------------------------------------------------------------
PARTS = 3
PER = 2 * CHUNK + 5                      # three parts per sample


def _sequences(N, steps, off, seed):
    """f [steps + 1, N] fp32 and norm parts [steps + 1, N, 3, 4] float64 (the last row feeds the closing form); sample n follows
    pattern (n + off) % 5: never adversarial; adversarial from k = 0 at distance 0; found, lost and found again in runs of two,
    the later finds closer; a random walk that drifts down, with NaNs in it; never adversarial with a tiny gradient, so that
    worst caps eps.  The count entries are integers."""
    gen = torch.Generator().manual_seed(seed)
    k = torch.arange(steps + 1, dtype=torch.float32)
    f = torch.empty(steps + 1, N)
    parts = torch.rand(steps + 1, N, PARTS, 4, generator=gen, dtype=torch.float64)
    parts[..., GSS] = parts[..., GSS] * 4.0 + 0.5
    parts[..., GMAX] = parts[..., GMAX] * 0.4 + 0.05
    parts[..., DABS] = parts[..., DABS] * 3.0
    parts[..., DCNT] = torch.floor(parts[..., DCNT] * 12.0)
    for n in range(N):
        p = (n + off) % 5
        base = float(torch.rand(1, generator=gen)) + 0.5
        if p == 0:
            f[:, n] = base / (1.0 + k)
        elif p == 1:
            f[:, n] = -base
            parts[0, n, :, DABS:] = 0.0
        elif p == 2:
            f[:, n] = base * torch.where((k // 2) % 2 == 0, 1.0, -1.0)
            shrink = (1.0 / (1.0 + 0.2 * k)).reshape(-1, 1).double()
            parts[:, n, :, DABS] *= shrink
            parts[:, n, :, DCNT] = torch.floor(parts[:, n, :, DCNT] * shrink)
        elif p == 3:
            f[:, n] = 0.3 + 0.05 * torch.randn(steps + 1, generator=gen).cumsum(0) - 0.02 * k
            f[1::4, n] = NAN                                                  # k = 1: NaN, nothing found yet
        else:
            f[:, n] = base
            parts[:, n, :, GSS] *= 1e-6
            parts[:, n, :, GMAX] *= 1e-4
    return f.contiguous(), parts.contiguous()


def _control_state(N, steps, dev):
    from unidefense_amd import kernels as K
    ist, fst = K.sfmn_state(N, dev)
    ist[1:].fill_(77)                                                      # k == 0 must initialise everything it reads later
    fst.fill_(-3.0)
    fac = torch.full((N,), -9.0, dtype=torch.float64, device=dev)
    hist = torch.full((steps + 1, N), -5.0, device=dev)
    ehist = torch.full((steps, N), -6.0, device=dev)
    return ist, fst, fac, hist, ehist


def _assert_state(ref, ist, fst, fac, where):
    i, fl, fc = ist.cpu().numpy(), fst.cpu().numpy(), fac.cpu().numpy()
    assert _same(i[0], ref.k) and _same(i[1], ref.found) and _same(i[2], ref.improved), where
    assert _same(fl[0], np.asarray(ref.eps, dtype=np.float32)) and _same(fl[1], np.asarray(ref.best, dtype=np.float32)), where
    assert _same(fc, ref.fac), where


def _worst(N, norm, seed):
    gen = torch.Generator().manual_seed(seed)
    if norm == "l0":
        return torch.floor(torch.rand(N, generator=gen) * 20.0 + 25.0).float()          # an integer, as per is
    return (torch.rand(N, generator=gen) * 4.0 + 6.0).float()


@pytest.mark.parametrize("norm", ["l1", "l0"])
@pytest.mark.parametrize("steps", [5, 100])
@pytest.mark.parametrize("N", [1, 7, 300])
def test_control_vs_reference_step_by_step(N, steps, norm):
    from unidefense_amd import kernels as K
    from unidefense_amd.attack import fmn_schedule
    dev = _dev()
    alpha, gamma = fmn_schedule(steps)
    worst = _worst(N, norm, N + steps)
    seen = {"adv": 0, "lost": 0, "far": 0, "capped": 0, "nan": 0, "floored": 0, "improved_later": 0, "closing_improved": 0}
    for off in (range(5) if N == 1 else (0,)):
        f, parts = _sequences(N, steps, off, 11 * N + steps + off)
        fd, pd = f.to(dev), parts.to(dev)
        ist, fst, fac, hist, ehist = _control_state(N, steps, dev)
        ist[K.SFMN_I["k"]].zero_()
        ref = ref_sfmn_control(N, steps, norm, alpha.tolist(), gamma.tolist(), worst.tolist(), width=HI - LO)
        args = (alpha.to(dev), gamma.to(dev), worst.to(dev), norm, LO, HI)
        for k in range(steps):
            K.sfmn_control(fd[k], pd[k], PER, ist, fst, fac, hist, ehist, *args)
            ref.step(f[k].tolist(), parts[k].numpy())
            _assert_state(ref, ist, fst, fac, (N, steps, norm, off, k))
            if k > 0:
                seen["improved_later"] += sum(ref.improved)
        h, eh = hist.cpu().numpy(), ehist.cpu().numpy()
        assert _same(h[:steps], f[:steps].numpy()) and _same(h[steps], [-5.0] * N)
        assert _same(eh, np.asarray(ref.eps_history, dtype=np.float32))
        if norm == "l0":
            assert bool(np.all((eh == np.floor(eh)) | np.isinf(eh)))                   # an l0 budget is an integer or inf
        snap = [t.clone() for t in (ist, fst, fac, hist, ehist)]                       # past the last iteration: nothing moves
        K.sfmn_control(fd[0], pd[0], PER, ist, fst, fac, hist, ehist, *args)
        for t, s in zip((ist, fst, fac, hist, ehist), snap):
            assert _same(t.cpu().numpy(), s.cpu().numpy())
        K.sfmn_control(fd[steps], pd[steps], PER, ist, fst, fac, hist, ehist, *args, closing=True)
        ref.close(f[steps].tolist(), parts[steps].numpy())
        _assert_state(ref, ist, fst, fac, (N, steps, norm, off, "closing"))
        assert _same(hist.cpu().numpy(), np.asarray(ref.history, dtype=np.float32))
        assert _same(ehist.cpu().numpy(), eh)
        seen["closing_improved"] += sum(ref.improved)
        for b in ("adv", "lost", "far", "capped", "nan", "floored"):
            seen[b] += ref.branch[b]
    print(f"  control N {N} steps {steps} {norm}: {seen}")
    assert all(seen[b] > 0 for b in ("adv", "lost", "far", "capped", "nan", "improved_later")), (N, steps, norm, seen)
    if norm == "l0":
        assert seen["floored"] > 0, seen       # pattern 1 stays adversarial at eps 0: min(floor(0), 0 - 1) = -1 is raised to 0


def test_control_is_restartable():
    """zeroing the counter row starts a new run on the same buffers; two runs on the same sequence give the same state"""
    from unidefense_amd import kernels as K
    from unidefense_amd.attack import fmn_schedule
    dev = _dev()
    N, steps = 130, 10
    alpha, gamma = (t.to(dev) for t in fmn_schedule(steps))
    f, parts = _sequences(N, steps, 0, 5)
    f, parts = f.to(dev), parts.to(dev)
    ist, fst, fac, hist, ehist = _control_state(N, steps, dev)
    for norm in ("l1", "l0"):
        worst = _worst(N, norm, 3).to(dev)
        snaps = []
        for _ in range(2):
            ist[K.SFMN_I["k"]].zero_()
            for k in range(steps):
                K.sfmn_control(f[k], parts[k], PER, ist, fst, fac, hist, ehist, alpha, gamma, worst, norm, LO, HI)
            K.sfmn_control(f[steps], parts[steps], PER, ist, fst, fac, hist, ehist, alpha, gamma, worst, norm, LO, HI, closing=True)
            snaps.append([t.clone() for t in (ist, fst, fac, hist, ehist)])
        for a, b in zip(*snaps):
            assert _same(a.cpu().numpy(), b.cpu().numpy())
        assert int(snaps[0][0][K.SFMN_I["found"]].sum()) > 0


# ---- 3. ud_sfmn_select + ud_sfmn_apply vs the float64 projections ------------------------------------------------------------
FILLS = ("random", "quantised", "zeros", "large")
SHAPES = [(1, 1), (1, 3), (8, 5), (3, 4099), (2, 3 * 32 * 32), (2, 3 * 64 * 64 + 1)]


def _proj_case(N, per, fill, seed):
    """x0, x, x_best, g fp32 [N, per] and fac [N]: random; quantised: everything a multiple of 1/8 and fac = 1, so z - x0 is
    exact and full of ties; zeros: x = x0 and g zero but for one element in eleven; large: a step that leaves the clip box"""
    gen = torch.Generator().manual_seed(seed)
    x0 = torch.rand(N, per, generator=gen) * 2 - 1
    x = (x0 + (torch.rand(N, per, generator=gen) * 2 - 1) * 0.1).clamp(LO, HI)
    x_best = (x0 + (torch.rand(N, per, generator=gen) * 2 - 1) * 0.1).clamp(LO, HI)
    g = torch.randn(N, per, generator=gen)
    fac = [(0.7, 0.01, 0.3, 0.05)[n % 4] for n in range(N)]
    if fill == "quantised":
        x0, x, g = (torch.round(t * 8.0) / 8.0 for t in (x0, x, g))
        fac = [1.0] * N
    elif fill == "zeros":
        x = x0.clone()
        mask = torch.zeros(N * per, dtype=torch.bool)
        mask[::11] = True
        g = torch.where(mask.reshape(N, per), g, torch.zeros(()))
    elif fill == "large":
        fac = [(50.0, 7.0, 200.0)[n % 3] for n in range(N)]
    return x0, x, x_best, g, fac


def _z32(x, g, fac):
    """the kernels' z: product and difference in double, one rounding to fp32"""
    return (x.double() - g.double() * torch.tensor(fac, dtype=torch.float64).reshape(-1, 1)).float()


def _budgets(norm, a_sum, per, N, off):
    """a budget per sample, rotated by off: 0, inf, larger than the norm, a mid value, a small one; l0 also kk = 1, per - 1, per"""
    out = []
    for n in range(N):
        j = (n + off)
        if norm == "l1":
            s = float(a_sum[n])
            out.append((0.0, INF, 2.0 * s + 1.0, 0.3 * s, 0.02 * s)[j % 5])
        else:
            out.append((0.0, INF, float(per + 5), float(per // 3), 1.0, float(per - 1), float(per))[j % 7])
    return [float(np.float32(e)) for e in out]


def _launch(norm, x, x_best, x0, g, improved, eps, fac, dev):
    from unidefense_amd import kernels as K
    N = x.shape[0]
    ist, fst = K.sfmn_state(N, dev)
    ist[K.SFMN_I["improved"]] = torch.tensor(improved, dtype=torch.int32, device=dev)
    fst[K.SFMN_F["eps"]] = torch.tensor(eps, dtype=torch.float32, device=dev)
    fst[K.SFMN_F["best"]].fill_(NAN)                                       # never read here
    facd = torch.tensor(fac, dtype=torch.float64, device=dev)
    thr = torch.full((N,), -77.0, dtype=torch.float64, device=dev)
    xd, xbd, x0d, gd = x.clone().to(dev), x_best.clone().to(dev), x0.to(dev), g.to(dev)
    K.sfmn_select(xd, x0d, gd, fst, facd, thr, norm)
    K.sfmn_apply(xd, xbd, x0d, gd, ist, facd, thr, norm, LO, HI)
    torch.cuda.synchronize()
    return xd.cpu(), xbd.cpu(), thr.cpu()


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("N,per", SHAPES)
def test_select_and_apply_l0_exact(N, per, fill):
    """the kept set is the reference's, kept elements are bitwise clamp(z), dropped ones bitwise clamp(x0); x_best is bitwise the
    old x where improved and untouched elsewhere; a second launch gives the same bits"""
    dev = _dev()
    x0, x, x_best, g, fac = _proj_case(N, per, fill, 7 * per + N)
    z = _z32(x, g, fac)
    improved = [n & 1 for n in range(N)]
    for off in (range(7) if N == 1 else range(0, 7, 3) if N < 7 else (0,)):
        eps = _budgets("l0", None, per, N, off)
        got, got_best, thr = _launch("l0", x, x_best, x0, g, improved, eps, fac, dev)
        ref, kept = ref_project_l0(z, x0, eps, LO, HI)
        want = torch.where(kept, z.clamp(LO, HI), x0.clamp(LO, HI))
        assert torch.equal(want.double(), ref)                                       # fp32 values: the float64 reference exactly
        assert torch.equal(got != x0.clamp(LO, HI), want != x0.clamp(LO, HI)), (N, per, fill, off)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (N, per, fill, off, int((got != want).sum()))
        for n in range(N):
            kk = eps[n]
            if kk == INF or kk >= per:
                assert float(thr[n]) == -1.0 and torch.equal(got[n].view(torch.int32), z[n].clamp(LO, HI).view(torch.int32))
            elif kk == 0.0:
                assert float(thr[n]) == INF and int(kept[n].sum()) == 0        # nothing is above +inf: the sample is not read
            else:
                assert int(kept[n].sum()) <= int(kk)
                a = (z[n].double() - x0[n].double()).abs()
                assert float(thr[n]) == float(torch.sort(a, descending=True).values[int(kk)])
            if kk == 0.0:
                assert torch.equal(got[n], x0[n].clamp(LO, HI))
        assert torch.equal(got_best, torch.where(torch.tensor(improved).bool().reshape(-1, 1), x, x_best))
        again = _launch("l0", x, x_best, x0, g, improved, eps, fac, dev)
        assert all(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a.view(torch.int32),
                               b.view(torch.int64) if b.dtype == torch.float64 else b.view(torch.int32))
                   for a, b in zip((got, got_best, thr), again))


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("N,per", SHAPES)
def test_select_and_apply_l1_vs_float64(N, per, fill):
    """every element within 2^-22 max(1, |ref|) of the sort-based float64 reference rounded to fp32 (tau in double is good to
    ~1e-10 relative: only the last rounding can differ); sum |x - x0| in float64 <= eps + per 2^-24 max(|lo|, |hi|); the
    no-projection cases are bitwise clamp(z); eps = 0 gives clamp(x0); x_best and the second launch as for l0"""
    dev = _dev()
    x0, x, x_best, g, fac = _proj_case(N, per, fill, 5 * per + N)
    z = _z32(x, g, fac)
    a_sum = (z.double() - x0.double()).abs().sum(1)
    improved = [(n + 1) & 1 for n in range(N)]
    worst_d = worst_s = 0.0
    for off in (range(5) if N < 5 else (0,)):
        eps = _budgets("l1", a_sum, per, N, off)
        got, got_best, thr = _launch("l1", x, x_best, x0, g, improved, eps, fac, dev)
        ref = ref_project_l1(z, x0, eps, LO, HI)
        want = ref.float()
        tol = 2.0 ** -22 * torch.clamp(want.abs(), min=1.0)
        d = (got - want).abs()
        worst_d = max(worst_d, float((d / tol).max()))
        assert bool((d <= tol).all()), (N, per, fill, off, float((d / tol).max()))
        for n in range(N):
            e = eps[n]
            if e == INF or float(a_sum[n]) <= e:
                assert float(thr[n]) == -1.0
                assert torch.equal(got[n].view(torch.int32), z[n].clamp(LO, HI).view(torch.int32)), (n, e)
            else:
                assert float(thr[n]) >= 0.0
                s = float((got[n].double() - x0[n].double()).abs().sum())
                worst_s = max(worst_s, s - e)
                assert s <= e + per * 2.0 ** -24 * max(abs(LO), abs(HI)), (n, e, s)
            if e == 0.0 and float(a_sum[n]) > 0.0:
                assert float(thr[n]) == INF and torch.equal(got[n], x0[n].clamp(LO, HI))
        assert torch.equal(got_best, torch.where(torch.tensor(improved).bool().reshape(-1, 1), x, x_best))
        again = _launch("l1", x, x_best, x0, g, improved, eps, fac, dev)
        assert torch.equal(got.view(torch.int32), again[0].view(torch.int32)) and torch.equal(got_best, again[1])
        assert torch.equal(thr.view(torch.int64), again[2].view(torch.int64))
    within(f"ud_sfmn_select+apply l1 N {N} per {per} {fill}: max |x - ref| / (2^-22 max(1, |ref|))", worst_d, 1.0)
    print(f"  l1 N {N} per {per} {fill}: max |x - ref| / bar {worst_d:.3f}; max (sum |x - x0| - eps) {worst_s:.3e}")


@pytest.mark.parametrize("norm", ["l1", "l0"])
def test_a_nan_gradient_element_stays_in_its_sample(norm):
    """one NaN gradient element in one sample: the launch returns, that sample's x is not finite at least at that element, and
    every other sample is bitwise what it is without the NaN"""
    dev = _dev()
    N, per = 4, 3 * 64 * 64 + 1
    x0, x, x_best, g, fac = _proj_case(N, per, "random", 3)
    z = _z32(x, g, fac)
    a_sum = (z.double() - x0.double()).abs().sum(1)
    improved = [1, 0, 1, 0]
    eps = [float(np.float32(0.3 * float(a_sum[n]))) for n in range(N)] if norm == "l1" else [float(per // 3)] * N
    clean = _launch(norm, x, x_best, x0, g, improved, eps, fac, dev)
    for at in (0, per // 2, per - 1):
        gb = g.clone()
        gb[2, at] = NAN
        got = _launch(norm, x, x_best, x0, gb, improved, eps, fac, dev)
        assert not bool(torch.isfinite(got[0][2, at]))
        for n in (0, 1, 3):
            assert torch.equal(got[0][n].view(torch.int32), clean[0][n].view(torch.int32))
            assert float(got[2][n]) == float(clean[2][n])
        assert torch.equal(got[1], clean[1])


# ---- 4. the runner: exact properties -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["l1", "l0"])
@pytest.mark.parametrize("name,size,n,seed,steps", [("UDR18", 128, 2, 5, 1), ("UDR18", 128, 2, 5, 3), ("UDR18", 128, 2, 5, 10),
                                                    ("UDEB4", 256, 2, 7, 3)])
def test_sparse_fmn_runner_exact_properties(name, size, n, seed, steps, norm):
    from unidefense_amd.attack import SparseFMNRunner
    dev = _dev()
    m = _shared(name, dev)
    x = param_fill.make_input(n, size, seed).to(dev)
    y = param_fill.make_labels(n).to(dev)
    per = 3 * size * size
    assert float(x.min()) >= LO and float(x.max()) <= HI
    r = SparseFMNRunner(m, n, size, norm=norm, steps=steps, alpha_init=ALPHA[norm])
    assert r.args["method"] == "sparse_fmn" and r.args["steps"] == steps and r.args["norm"] == norm
    assert r.args["alpha_init"] == ALPHA[norm] and r.args["alpha_final"] == ALPHA[norm] / 100.0 and r.args["objective"] == "margin"
    warm = r(x, y).clone()
    assert r.graph is None
    runs = []
    for _ in range(2):
        xa = r(x, y)
        runs.append([t.clone() for t in (xa, r.radius, r.found, r.history, r.eps_history, r.margin0)])
    torch.cuda.synchronize()
    assert r.graph is not None and r.closing_graph is not None and xa is r.x_adv
    for a, b in zip(*runs):
        assert _same(a.cpu().numpy(), b.cpu().numpy())                    # two replays: the same bits (inf included)
    xa, radius, found, hist, ehist, margin0 = runs[0]
    assert radius.dtype == torch.float32 and found.dtype == torch.int32
    assert tuple(radius.shape) == tuple(found.shape) == tuple(margin0.shape) == (n,)
    assert tuple(hist.shape) == (steps + 1, n) and tuple(ehist.shape) == (steps, n) and torch.equal(margin0, hist[0])
    assert tuple(r.g.shape) == tuple(x.shape) and set(r.out) == {"cls_out", "rec", "loss_dict"}
    print(f"  sparse FMN {name} {norm} steps {steps}: radius {radius.tolist()}  found {found.tolist()}  margin0 {margin0.tolist()}")
    print(f"    history {[[round(float(v), 5) for v in row] for row in hist]}")
    print(f"    eps_history {[[round(float(v), 5) for v in row] for row in ehist]}")
    assert torch.isfinite(hist).all()
    for out in (warm, xa):
        assert torch.isfinite(out).all() and float(out.min()) >= LO and float(out.max()) <= HI
    assert torch.equal(found.bool(), torch.isfinite(radius))
    d = (xa.cpu().double() - x.cpu().double()).flatten(1)
    for i in range(n):
        if found[i]:
            if norm == "l0":
                assert float(radius[i]) == float((xa[i] != x[i]).sum()), (i, float(radius[i]))
            else:
                got = float(d[i].abs().sum())
                rel = abs(float(radius[i]) - got) / got if got > 0 else float(radius[i])
                assert within(f"SparseFMNRunner {name} l1 steps {steps}: radius vs sum |x_adv - x| in float64, rel", rel, 1e-6)
        else:
            assert torch.equal(xa[i], x[i])                              # nothing found: the input, untouched
        if float(margin0[i]) < 0:                                       # misclassified as it is: radius 0, the clamped input
            assert found[i] and float(radius[i]) == 0.0 and torch.equal(xa[i], x[i].clamp(LO, HI))
    # eps never exceeds the cap; an l0 budget is an integer
    worst = r._worst.cpu()
    want_worst = torch.tensor(ref_sfmn_worst(x.cpu().double(), norm, LO, HI))
    assert bool(((worst.double() - want_worst).abs() <= 1e-6 * want_worst).all()) and (norm == "l1" or bool((worst == per).all()))
    assert bool((ehist.cpu() <= worst.reshape(1, -1)).all())
    if norm == "l0":
        assert bool((ehist == torch.floor(ehist)).all())
    if name == "UDR18":
        assert [bool(v < 0) for v in margin0] == [True, False], margin0   # the float64 oracle: margin0 -2.67 and +3.45
    within(f"SparseFMNRunner {name} {norm} steps {steps}: replay vs eager warm-up x_adv, max|d| (recorded)",
           float((xa - warm).abs().max()), 2.0)


# ---- 5. the objective at x_adv -----------------------------------------------------------------------------------------------
OBJECTIVE_CASES = [("UDR18", 128, 2, 5, "l1", 10, "fp32"), ("UDR18", 128, 2, 5, "l0", 20, "fp32"),
                   ("UDEB4", 256, 2, 7, "l1", 6, "fp16")]


@pytest.mark.parametrize("name,size,n,seed,norm,steps,precision", OBJECTIVE_CASES)
def test_objective_at_x_adv_is_the_one_its_best_was_set_at(name, size, n, seed, norm, steps, precision):
    """tests/test_n_fmn_gpu.py's test of the same name, its method and its bar: the eager first call records the iteration at
    which `improved` last fired for each sample; the objective that the same-precision forward gives at x_adv is THAT row of
    history within 1e-5 max|cls_out|, and that row is negative.  The UDR18 cases are the effect test's: every sample is found,
    one at a distance.  The UDEB4 case runs the half-storage pass on the confidence-threshold objective of the FMN suite
    (margin - 0.9394, f0 = +0.00201 / -1.8826): the float64 reference finds sample 1 (as it is) and NOT sample 0 in 6 steps in
    either sparse norm at alpha_init 32, 128 or 256 (f stays at 0.0015 .. 0.0045: a few pixels moved across the whole clip box
    leave the linear regime of the param-filled UDEB4), so there the check holds for whichever samples the GPU found."""
    from unidefense_amd.attack import SparseFMNRunner
    from unidefense_amd.infer import InferenceRunner
    dev = _dev()
    m = _shared(name, dev)
    x = param_fill.make_input(n, size, seed).to(dev)
    y = param_fill.make_labels(n).to(dev)
    kw = dict(objective=_eb4_objective) if name == "UDEB4" else {}
    r = SparseFMNRunner(m, n, size, norm=norm, steps=steps, precision=precision, alpha_init=EB4_ALPHA if name == "UDEB4" else ALPHA[norm],
                        **kw)
    fired, control = [], r._control

    def recording(f, closing=False):
        control(f, closing=closing)
        fired.append(r._improved.clone())
    r._control = recording
    xa = r(x, y).clone()                                   # the eager call: one control launch per iteration, then the closing one
    del r._control
    assert len(fired) == steps + 1 and r.graph is None
    fired, hist = torch.stack(fired).cpu(), r.history.clone()
    with torch.no_grad():
        if precision == "fp32":
            out = m(xa)
        else:
            inf = InferenceRunner(m, n, size, "fp16")
            inf(xa)
            out = inf(xa)
        mg = r.objective(out, y)
        scale = float(out["cls_out"].abs().max())
    found = r.found.bool()
    if name == "UDR18":
        assert bool(found.all()) and bool((r.radius > 0).any())      # every sample found, at least one at a distance
    assert bool(found.any()) and torch.equal(fired.any(0), found.cpu())
    for i in range(n):
        if not found[i]:
            assert torch.equal(xa[i], x[i])
            continue
        k = int(fired[:, i].nonzero().max())
        d = abs(float(hist[k, i]) - float(mg[i]))
        print(f"  sparse FMN {name} {norm} {precision} sample {i}: best set at k = {k}, objective(x_adv) {float(mg[i]):.6g}, "
              f"history[{k}] {float(hist[k, i]):.6g}, |d| / max|cls_out| {d / scale:.2e}, radius {float(r.radius[i]):.6g}")
        assert float(hist[k, i]) < 0
        assert within(f"SparseFMNRunner {name} {norm} {precision}: objective of the forward at x_adv vs history at the iteration "
                      f"that set best, |d| / max|cls_out|", d / scale, 1e-5)
    xb = r(x, y)                                           # the capture and the first replay: the same attack
    assert r.graph is not None
    within(f"SparseFMNRunner {name} {norm} {precision}: replay vs eager x_adv, max|d| (recorded)", float((xb - xa).abs().max()), 2.0)


# ---- 6. effect, judged by the oracle -----------------------------------------------------------------------------------------
# ref_sparse_fmn run entirely in the float64 oracle (margin_each on the oracle's forward), checked on the CPU first:
#   UDR18 128^2 n=2 seed 5, margin0 -2.6738 / +3.4458:
#     l1, steps 10, alpha_init 8  : found both; radii 0 and 133.606; sample 1: f 3.4458, 2.1432, 1.1417, 0.5195, 0.1895, 0.0389,
#       -0.0208 (k = 6), -0.0130, -0.0057, -0.0022, closing -0.0010; eps 56.67, 100.18, 125.18, 136.18, 138.94, 138.71, 136.22,
#       134.71, 133.95, 133.65; best set at the closing point
#     l0, steps 20, alpha_init 256: found both; radii 0 and 141 of 49 152 elements; f crosses at k = 12 (0.1856 -> -0.2848);
#       eps 29, 54, 72, 87, 101, 116, 126, 135, 142, 148, 153, 155, 152, 149, 147, 145, 144, 143, 142, 141
#   (alpha_init 1 does not cross in 10 steps in l1, nor 8 or 64 in l0: the L2-normalised step must be sized to the norm)
EB4_ALPHA = 32.0
EFFECT = [("UDR18", 128, 2, 5, "l1", 10), ("UDR18", 128, 2, 5, "l0", 20)]


@functools.lru_cache(maxsize=None)
def _oracle_sparse_fmn(name, size, n, seed, norm, steps):
    from unidefense_amd.attack import margin_each
    x = param_fill.make_input(n, size, seed)
    y = param_fill.make_labels(n)

    def fg(x64, need_grad):
        if not need_grad:
            with torch.no_grad():
                return margin_each(_oracle_fwd(name, x64), y), None
        xg = x64.detach().clone().requires_grad_()
        f = margin_each(_oracle_fwd(name, xg), y)
        g, = torch.autograd.grad(f.sum(), xg)
        return f.detach(), g
    return ref_sparse_fmn(fg, x, norm, steps, alpha_init=ALPHA[norm], lo=LO, hi=HI)


@pytest.mark.parametrize("name,size,n,seed,norm,steps", EFFECT)
def test_sparse_fmn_effect_judged_by_the_oracle(name, size, n, seed, norm, steps):
    """As tests/test_n_fmn_gpu.py::test_fmn_effect_judged_by_the_oracle: the reference finds every sample, at least one at a
    distance; the GPU finds each sample the reference finds; radius_gpu / radius_ref - 1 <= (1 + gamma0) / (1 - gamma0) - 1; the
    ORACLE's objective at the GPU's x_adv is at most 1e-3 max|cls_out64|.  Reference radii, observed on the CPU: 0 and 133.606
    (l1), 0 and 141 (l0).  Observed on the GPU: DESIGN 3q."""
    from unidefense_amd.attack import SparseFMNRunner, margin_each
    dev = _dev()
    m = _shared(name, dev)
    x = param_fill.make_input(n, size, seed)
    y = param_fill.make_labels(n)
    r = SparseFMNRunner(m, n, size, norm=norm, steps=steps, alpha_init=ALPHA[norm])
    r(x.to(dev), y.to(dev))
    xa = r(x.to(dev), y.to(dev)).cpu()
    radius, found = r.radius.cpu().double(), r.found.cpu().bool()
    ref = _oracle_sparse_fmn(name, size, n, seed, norm, steps)
    with torch.no_grad():
        out64 = _oracle_fwd(name, xa.double())
        m64 = margin_each(out64, y)
        scale = float(out64["cls_out"].abs().max())
    print(f"  sparse FMN {name} {norm} steps {steps}: radius gpu {radius.tolist()}  ref {ref['radius'].tolist()}  found gpu "
          f"{found.tolist()} ref {ref['found']}  best set at (ref) {ref['best_at']}")
    print(f"    f64(x_adv) {m64.tolist()}  max|cls_out64| {scale:.4g}  f0 gpu {r.margin0.tolist()} ref {ref['history'][0]}")
    print(f"    oracle eps_history {[[round(v, 4) for v in row] for row in ref['eps_history']]}")
    print(f"    gpu eps_history    {[[round(float(v), 4) for v in row] for row in r.eps_history]}")
    print(f"    oracle history {[[round(v, 6) for v in row] for row in ref['history']]}")
    print(f"    gpu history    {[[round(float(v), 6) for v in row] for row in r.history]}")
    assert ref["found"] == [1] * n                        # the fixture's premise: the reference finds every sample
    assert any(float(v) > 0 for v in ref["radius"])       # and at least one of them at a distance
    ok = []
    for i in range(n):
        assert bool(found[i]), (i, "the reference found this sample, the GPU did not")
        rr = float(ref["radius"][i])
        ratio = float(radius[i]) / rr - 1.0 if rr > 0 else (0.0 if float(radius[i]) == 0.0 else INF)
        ok.append(within(f"sparse FMN effect {name} {norm} steps {steps}: radius_gpu / radius_ref - 1", ratio, ONE_DECISION))
        ok.append(within(f"sparse FMN effect {name} {norm} steps {steps}: oracle objective at x_adv / (1e-3 max|cls_out64|)",
                         float(m64[i]) / (1e-3 * scale), 1.0))
    assert all(ok), (radius, ref["radius"], m64, scale)


# ---- 7. what the runner leaves alone -----------------------------------------------------------------------------------------
def test_sparse_fmn_leaves_the_model_and_the_other_runners_as_they_were():
    from unidefense_amd import lib
    from unidefense_amd.attack import AttackRunner, FMNRunner, SparseFMNRunner
    dev = _dev()
    n = 2
    x = param_fill.make_input(n, 256, 31).to(dev)
    y = param_fill.make_labels(n).to(dev)
    fresh = _build("UDEB4", dev)
    flags = _mixed_flags(fresh)
    _train_grads(fresh, x, y, dev)                   # the first step of a shape measures GEMM plans; the second runs on them
    want = _train_grads(fresh, x, y, dev)
    del fresh
    m = _build("UDEB4", dev).eval()
    assert _mixed_flags(m) == flags and not all(flags) and any(flags)
    bufs = {k: v.clone() for k, v in m.named_buffers()}
    pgd = AttackRunner(m, n, 256, norm="linf", eps=2.0 / 255.0, steps=2)
    fmn = m.fmn_runner(n, 256, norm="l2", steps=2)
    before = []
    for r in (pgd, fmn):
        r(x, y)
        before.append(r(x, y).clone())
        assert r.graph is not None
    slots = ("_ud_runners", "_ud_grad_runners", "_ud_attack_runners", "_ud_apgd_runners", "_ud_square_runners", "_ud_fmn_runners")
    caches = {k: dict(m.__dict__.get(k, {})) for k in slots}
    assert len(caches["_ud_fmn_runners"]) == 1
    path = lib.call("ud_gemm_get_path")
    for r in (SparseFMNRunner(m, n, 256, norm="l1", steps=3, alpha_init=8.0), SparseFMNRunner(m, n, 256, norm="l0", steps=3, alpha_init=256.0),
              m.sparse_fmn_runner(n, 256, steps=2)):
        for _ in range(3):
            r(x, y)
    torch.cuda.synchronize()
    assert lib.call("ud_gemm_get_path") == path
    assert len(m.__dict__["_ud_sparse_fmn_runners"]) == 1
    assert {k: dict(m.__dict__.get(k, {})) for k in caches} == caches
    assert [p.requires_grad for p in m.parameters()] == flags
    assert all(p.grad is None for p in m.parameters())
    assert not m.training
    now = dict(m.named_buffers())
    assert all(torch.equal(v, now[k]) for k, v in bufs.items())
    assert torch.equal(pgd(x, y), before[0]) and torch.equal(fmn(x, y), before[1])     # captured before: the same bits
    got = _train_grads(m, x, y, dev)
    assert got.keys() == want.keys() and len(got) > 300
    diff = [k for k in got if not torch.equal(got[k], want[k])]
    assert not diff, diff[:10]


def test_captured_sparse_fmn_runner_follows_an_optimizer_step():
    from unidefense_amd.attack import SparseFMNRunner
    dev = _dev()
    n = 2
    m = _build("UDEB4", dev).eval()
    x = param_fill.make_input(n, 256, 51).to(dev)
    y = param_fill.make_labels(n).to(dev)
    at = SparseFMNRunner(m, n, 256, norm="l1", steps=2, alpha_init=8.0)
    at(x, y)
    a0, h0 = at(x, y).clone(), at.history.clone()
    assert at.graph is not None
    torch.manual_seed(5)
    params = [p for p in m.parameters() if p.requires_grad]
    for p in params:
        p.grad = torch.randn_like(p) * 1e-2
    opt = torch.optim.AdamW(params, lr=1e-3)
    ptrs = [p.data_ptr() for p in params]
    opt.step()
    assert ptrs == [p.data_ptr() for p in params]
    m.zero_grad(set_to_none=True)
    bn = m.backbone._blocks[3]._bn0
    bn.running_mean.add_(0.05)
    bn.running_var.mul_(1.5)
    a1, h1, r1 = at(x, y).clone(), at.history.clone(), at.radius.clone()
    print(f"  history after / before the optimizer step, rel L2 {_rel_l2(h1, h0):.3e}")
    assert not torch.equal(h1, h0)                         # the step changed the function
    at2 = SparseFMNRunner(m, n, 256, norm="l1", steps=2, alpha_init=8.0)
    at2(x, y)
    assert torch.equal(a1, at2(x, y)) and torch.equal(h1, at2.history) and _same(r1.cpu().numpy(), at2.radius.cpu().numpy())


@pytest.mark.parametrize("norm", ["l1", "l0"])
def test_targeted_towards_the_other_class_is_the_untargeted_attack(norm):
    """-margin(out, 1 - y) = margin(out, y) on the two-class model: the same bits; and the call refusals of the shared body"""
    from unidefense_amd.attack import SparseFMNRunner
    dev = _dev()
    m = _shared("UDR18", dev)
    x = param_fill.make_input(2, 128, 5).to(dev)
    y = param_fill.make_labels(2).to(dev)
    r = SparseFMNRunner(m, 2, 128, norm=norm, steps=1)
    with pytest.raises(ValueError, match="cuda"):
        r(x.cpu(), y)
    with pytest.raises(ValueError, match="differs"):
        r(x[:1], y)
    assert r.calls == 0
    plain = SparseFMNRunner(m, 2, 128, norm=norm, steps=3, alpha_init=ALPHA[norm])
    plain(x, y)
    a = plain(x, y).clone()
    tgt = SparseFMNRunner(m, 2, 128, norm=norm, steps=3, alpha_init=ALPHA[norm], targeted=True)
    tgt(x, 1 - y)
    assert torch.equal(tgt(x, 1 - y), a) and torch.equal(tgt.radius, plain.radius) and torch.equal(tgt.history, plain.history)
    assert torch.equal(tgt.eps_history, plain.eps_history)


# ---- 8. the engine -----------------------------------------------------------------------------------------------------------
def test_engine_test_robust_sparse_fmn():
    _dev()
    from tests.test_d_train_engine import CONFIG
    from unidefense_amd.attack import robust_curve
    from unidefense_amd.engine import get_engine
    cfg = copy.deepcopy(CONFIG)
    cfg["model"] = {"name": "UDR18", "num_classes": 2, "drop_rate": 0.2}
    cfg["data"] = {"train_batch_size": 2, "size": 128}
    eng = get_engine("FE")(cfg, "Test")
    param_fill.fill_module_(eng.model_without_ddp, sf_coef=0.0, fuse_coef=0.3)
    t0 = eng.test(batches=2)
    attack = {"method": "sparse_fmn", "norm": "l1", "steps": 5, "alpha_init": 8.0, "eps": 0.0}
    eng.test_robust(batches=2, attack=attack)                                   # the eager warm-up and the capture
    res = eng.test_robust(batches=2, attack=attack)
    assert attack == {"method": "sparse_fmn", "norm": "l1", "steps": 5, "alpha_init": 8.0, "eps": 0.0}     # not consumed
    assert set(res) == {"clean", "adv", "attack"}
    runner_args = eng.model_without_ddp.sparse_fmn_runner(res["clean"]["scores"].numel() // 2, 128, norm="l1", steps=5,
                                                          alpha_init=8.0).args
    assert set(res["attack"]) == set(runner_args) | {"eps", "radius", "found", "median_radius"}
    assert {k: res["attack"][k] for k in runner_args} == runner_args and res["attack"]["method"] == "sparse_fmn"
    assert res["attack"]["eps"] == 0.0 and res["attack"]["steps"] == 5 and res["attack"]["norm"] == "l1"
    assert not eng.model_without_ddp.__dict__.get("_ud_fmn_runners")
    _same_result(res["clean"], t0)
    radius, found = res["attack"]["radius"], res["attack"]["found"]
    ns = res["clean"]["scores"].numel()
    assert not radius.is_cuda and not found.is_cuda and tuple(radius.shape) == tuple(found.shape) == (ns,)
    assert torch.equal(found.bool(), torch.isfinite(radius))
    assert res["attack"]["median_radius"] == float(radius.double().median())
    # eps = 0: only a sample that is adversarial as it is (radius 0: x_adv = clamp(x) = x) is taken — the clean scores, bitwise
    assert torch.equal(res["adv"]["scores"], res["clean"]["scores"])
    assert torch.equal(res["adv"]["labels"], res["clean"]["labels"])
    free = eng.test_robust(batches=2, attack={"method": "sparse_fmn", "norm": "l1", "steps": 5, "alpha_init": 8.0})
    assert free["attack"]["eps"] is None and _same(free["attack"]["radius"].numpy(), radius.numpy())
    _same_result(free["clean"], t0)
    clean, adv = _mean_ce(free["clean"]), _mean_ce(free["adv"])
    print(f"  radius {radius.tolist()}  found {found.tolist()}  mean cross-entropy of the scores: clean {clean:.4f}  adv {adv:.4f}")
    assert bool(found.any()) and adv >= clean
    med = res["attack"]["median_radius"]
    curve = robust_curve(radius, [0.0, med])
    assert float(curve[0]) == float((radius > 0).double().mean()) and float(curve[1]) == float((radius > med).double().mean())
    assert float(curve[0]) <= 1.0 - float((found.bool() & (radius == 0)).double().mean()) and float(curve[1]) <= float(curve[0])
    assert float(curve[1]) >= float((~found.bool()).double().mean())             # a sample never found is robust at every eps
    l0 = eng.test_robust(batches=1, attack={"method": "sparse_fmn", "norm": "l0", "steps": 3, "alpha_init": 256.0})
    r0 = l0["attack"]["radius"]
    assert bool(((r0 == torch.floor(r0)) | torch.isinf(r0)).all())               # numbers of elements
    with pytest.raises(ValueError, match="sparse_fmn") as err:
        eng.test_robust(batches=1, attack={"method": "cw", "eps": 0.1})
    assert all(name in str(err.value) for name in ("'pgd'", "'apgd'", "'square'", "'apgd+square'", "'fmn'"))
    with pytest.raises(ValueError, match="eps"):
        eng.test_robust(batches=1, attack={"method": "sparse_fmn", "eps": -1.0})
    _same_result(eng.test(batches=2), t0)
    assert all(p.grad is None for p in eng.model_without_ddp.parameters())
