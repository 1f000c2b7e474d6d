"""GPU: the Fast Minimum-Norm attack — the kernels of csrc/fmn.hip and the graph-replayed FMNRunner (unidefense_amd/attack.py;
TrainEngine.test_robust with "method": "fmn").

Kernels: ud_fmn_norm_parts against float64 numpy (sums to 1e-12 relative, the maximum exactly), ud_fmn_control step by step
against the numpy state machine of tests/test_fmn_cpu.py (every state array equal), ud_fmn_update bitwise against the torch
expression, ud_fmn_project_l2 bitwise against ud_attack_project_l2.  Runner: replay, clip, radius and found properties (exact),
consistency of the objective at x_adv with the forward, the EFFECT judged by the float64 oracle's margin at the GPU's x_adv and
by the radius against ref_fmn run entirely in the oracle, and what the runner must leave alone.

The trajectories (eps_history, history[1:]) are printed, never asserted: a near-tie decision (f < 0 on a value that differs from
zero in the last bits) is not reproducible between two correct evaluations."""
import copy
import functools

import numpy as np
import pytest
import torch

from oracle import eb4, param_fill
from tests import oracle_util as ou
from tests.margins import within
from tests.test_fmn_cpu import CHUNK, DMAX, DSS, GABS, GSS, ref_fmn, ref_fmn_control
from tests.test_j_attack_gpu import (_build, _mean_ce, _mixed_flags, _oracle_fwd, _rel_l2, _same_result, _shared, _train_grads)

pytestmark = pytest.mark.gpu

LO, HI = -1.0, 1.0
INF = float("inf")
NAN = float("nan")
GAMMA0 = 0.05


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    ou.fit_cpu_threads()
    return torch.device("cuda:0")


def _same(got, want):
    return np.array_equal(np.asarray(got), np.asarray(want), equal_nan=True)


# ---- 1. ud_fmn_norm_parts ----------------------------------------------------------------------------------------------------
def _norm_case(N, per, seed, shift):
    """x, x0, g fp32 [N, per] on the CPU; shift: every base is offset by one float from a 16-byte boundary"""
    gen = torch.Generator().manual_seed(seed)

    def make(scale):
        flat = torch.empty(N * per + 1)
        flat[shift:shift + N * per] = (torch.rand(N * per, generator=gen) * 2 - 1) * scale
        return flat
    return make(1.0), make(1.0), make(3.0)


def _view(flat, N, per, shift):
    return flat[shift:shift + N * per].view(N, per)


def _folded(parts):
    p = np.asarray(parts, dtype=np.float64)
    return p[:, :, GSS].sum(1), p[:, :, GABS].sum(1), p[:, :, DSS].sum(1), p[:, :, DMAX].max(1)


def _want_norms(x, x0, g):
    x, x0, g = (t.double().numpy() for t in (x, x0, g))
    d = x - x0
    return (g * g).sum(1), np.abs(g).sum(1), (d * d).sum(1), np.abs(d).max(1)


@pytest.mark.parametrize("per", [1, 5, 4096, 4097, 3 * 32 * 32])
@pytest.mark.parametrize("N", [1, 3])
def test_norm_parts_vs_float64(N, per):
    """the sums within 1e-12 relative of numpy's float64 (both add <= 4096 products of fp32 values per part in double: a relative
    error of at most ~4096 2^-53 = 5e-13 each way for these all-positive sums), the maximum exactly (the difference of two fp32
    values is exact in double).  shift 1 takes the scalar path at every per; g = None leaves the g entries as they were."""
    from unidefense_amd import kernels as K
    dev = _dev()
    parts = (per + CHUNK - 1) // CHUNK
    assert K.fmn_norms_ws_bytes(N, per) == N * parts * 32
    for shift in (0, 1):
        fx, fx0, fg = _norm_case(N, per, 13 * N + per + shift, shift)
        dx, dx0, dg = (_view(f.to(dev), N, per, shift) for f in (fx, fx0, fg))
        assert dx.data_ptr() % 16 == 4 * shift and dx.is_contiguous()
        ws = torch.full((N, parts, 4), -7.0, dtype=torch.float64, device=dev)
        K.fmn_norm_parts(dx, dx0, dg, ws=ws)
        got = _folded(ws.cpu().numpy())
        want = _want_norms(*(_view(f, N, per, shift) for f in (fx, fx0, fg)))
        for name, g_, w_ in zip(("sum g^2", "sum |g|", "sum d^2"), got[:3], want[:3]):
            rel = float(np.max(np.abs(g_ - w_) / np.maximum(np.abs(w_), 1e-300)))
            assert within(f"ud_fmn_norm_parts N {N} per {per} shift {shift}: {name} vs float64, max rel", rel, 1e-12)
        assert np.array_equal(got[3], want[3])
        # the default workspace (the scratch owner's) gives the same bits
        assert torch.equal(K.fmn_norm_parts(dx, dx0, dg), ws)
        # the closing form: the d entries again, the g entries untouched
        ws2 = torch.full((N, parts, 4), -7.0, dtype=torch.float64, device=dev)
        K.fmn_norm_parts(dx, dx0, None, ws=ws2)
        assert torch.equal(ws2[:, :, [DSS, DMAX]], ws[:, :, [DSS, DMAX]])
        assert bool((ws2[:, :, [GSS, GABS]] == -7.0).all())


@pytest.mark.parametrize("N,per", [(3, 5), (3, 4097), (3, 3 * 32 * 32)])
def test_norm_parts_keeps_a_nan_in_its_own_entries(N, per):
    """a NaN in x shows in the sample's two d entries (the maximum keeps it whichever thread, wave or part holds it) and
    nowhere else; a NaN in g shows in its two g entries only"""
    from unidefense_amd import kernels as K
    dev = _dev()
    fx, fx0, fg = _norm_case(N, per, per, 0)
    x, x0, g = (_view(f, N, per, 0).clone() for f in (fx, fx0, fg))
    clean = _folded(K.fmn_norm_parts(x.to(dev), x0.to(dev), g.to(dev)).cpu().numpy())
    for at in sorted({0, per // 2, per - 1}):
        xb = x.clone()
        xb[1, at] = NAN
        got = _folded(K.fmn_norm_parts(xb.to(dev), x0.to(dev), g.to(dev)).cpu().numpy())
        assert np.isnan(got[2][1]) and np.isnan(got[3][1]), at
        assert got[0][1] == clean[0][1] and got[1][1] == clean[1][1]
        for j in range(4):
            assert got[j][0] == clean[j][0] and got[j][2] == clean[j][2]
        gb = g.clone()
        gb[2, at] = NAN
        got = _folded(K.fmn_norm_parts(x.to(dev), x0.to(dev), gb.to(dev)).cpu().numpy())
        assert np.isnan(got[0][2]) and np.isnan(got[1][2]) and got[2][2] == clean[2][2] and got[3][2] == clean[3][2], at
        for j in range(4):
            assert got[j][0] == clean[j][0] and got[j][1] == clean[j][1]


# ---- 2. ud_fmn_control: every state array, step by step ----------------------------------------------------------------------
PARTS = 3
PER = 2 * CHUNK + 5                      # three parts per sample


def _sequences(N, steps, off, seed):
    """f [steps + 1, N] fp32 and norm parts [steps + 1, N, 3, 4] float64 (the last row feeds the closing form); sample n follows
    pattern (n + off) % 5: never adversarial; adversarial from k = 0 at distance 0; found, lost and found again in runs of two;
    a random walk that starts positive and drifts down, with NaNs in it; never adversarial with a tiny gradient, so that worst caps eps"""
    gen = torch.Generator().manual_seed(seed)
    k = torch.arange(steps + 1, dtype=torch.float32)
    f = torch.empty(steps + 1, N)
    parts = torch.rand(steps + 1, N, PARTS, 4, generator=gen, dtype=torch.float64)
    parts[..., GSS] = parts[..., GSS] * 4.0 + 0.5
    parts[..., GABS] = parts[..., GABS] * 40.0 + 5.0
    parts[..., DSS] = parts[..., DSS] * 0.01
    parts[..., DMAX] = parts[..., DMAX] * 0.05
    for n in range(N):
        p = (n + off) % 5
        base = float(torch.rand(1, generator=gen)) + 0.5
        if p == 0:
            f[:, n] = base / (1.0 + k)
        elif p == 1:
            f[:, n] = -base
            parts[0, n, :, DSS:] = 0.0
        elif p == 2:
            f[:, n] = base * torch.where((k // 2) % 2 == 0, 1.0, -1.0)
            parts[:, n, :, DSS] *= (1.0 / (1.0 + 0.2 * k)).reshape(-1, 1).double() ** 2      # the later finds are closer
            parts[:, n, :, DMAX] *= (1.0 / (1.0 + 0.2 * k)).reshape(-1, 1).double()
        elif p == 3:
            f[:, n] = 0.3 + 0.05 * torch.randn(steps + 1, generator=gen).cumsum(0) - 0.02 * k      # k = 1: NaN, nothing found yet
            f[1::4, n] = NAN
        else:
            f[:, n] = base
            parts[:, n, :, GSS] *= 1e-6
            parts[:, n, :, GABS] *= 1e-6
    return f.contiguous(), parts.contiguous()


def _control_state(N, steps, dev):
    from unidefense_amd import kernels as K
    ist, fst = K.fmn_state(N, dev)
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


@pytest.mark.parametrize("norm", ["linf", "l2"])
@pytest.mark.parametrize("steps", [5, 100])
@pytest.mark.parametrize("N", [1, 7, 300])
def test_control_vs_reference_step_by_step(N, steps, norm):
    from unidefense_amd import kernels as K
    from unidefense_amd.attack import fmn_schedule
    dev = _dev()
    alpha, gamma = fmn_schedule(steps)
    gen = torch.Generator().manual_seed(N + steps)
    worst = (torch.rand(N, generator=gen) * 0.2 + 0.2).float()
    seen = {"adv": 0, "lost": 0, "far": 0, "capped": 0, "nan": 0, "improved_later": 0, "closing_improved": 0}
    for off in (range(5) if N == 1 else (0,)):
        f, parts = _sequences(N, steps, off, 11 * N + steps + off)
        fd, pd = f.to(dev), parts.to(dev)
        ist, fst, fac, hist, ehist = _control_state(N, steps, dev)
        ist[K.FMN_I["k"]].zero_()
        ref = ref_fmn_control(N, steps, norm, alpha.tolist(), gamma.tolist(), worst.tolist())
        args = (alpha.to(dev), gamma.to(dev), worst.to(dev), norm)
        for k in range(steps):
            K.fmn_control(fd[k], pd[k], PER, ist, fst, fac, hist, ehist, *args)
            ref.step(f[k].tolist(), parts[k].numpy())
            _assert_state(ref, ist, fst, fac, (N, steps, norm, off, k))
            if k > 0:
                seen["improved_later"] += sum(ref.improved)
        h, eh = hist.cpu().numpy(), ehist.cpu().numpy()
        assert _same(h[:steps], f[:steps].numpy()) and _same(h[steps], [-5.0] * N)
        assert _same(eh, np.asarray(ref.eps_history, dtype=np.float32))
        # past the last iteration the kernel writes nothing
        snap = [t.clone() for t in (ist, fst, fac, hist, ehist)]
        K.fmn_control(fd[0], pd[0], PER, ist, fst, fac, hist, ehist, *args)
        for t, s in zip((ist, fst, fac, hist, ehist), snap):
            assert _same(t.cpu().numpy(), s.cpu().numpy())
        # the closing form: the keep-best decision, found and history[steps] only
        K.fmn_control(fd[steps], pd[steps], PER, ist, fst, fac, hist, ehist, *args, closing=True)
        ref.close(f[steps].tolist(), parts[steps].numpy())
        _assert_state(ref, ist, fst, fac, (N, steps, norm, off, "closing"))
        assert _same(hist.cpu().numpy(), np.asarray(ref.history, dtype=np.float32))
        assert _same(ehist.cpu().numpy(), eh)
        seen["closing_improved"] += sum(ref.improved)
        for b in ("adv", "lost", "far", "capped", "nan"):
            seen[b] += ref.branch[b]
    print(f"  control N {N} steps {steps} {norm}: {seen}")
    # the sequences make every branch of the eps rule fire (N == 1 walks through the five patterns one after the other)
    assert all(seen[b] > 0 for b in ("adv", "lost", "far", "capped", "nan", "improved_later")), (N, steps, norm, seen)


def test_control_is_restartable():
    """zeroing the counter row starts a new run on the same buffers; two runs on the same sequence give the same state"""
    from unidefense_amd import kernels as K
    from unidefense_amd.attack import fmn_schedule
    dev = _dev()
    N, steps = 130, 10
    alpha, gamma = (t.to(dev) for t in fmn_schedule(steps))
    worst = torch.full((N,), 0.3, device=dev)
    f, parts = _sequences(N, steps, 0, 5)
    f, parts = f.to(dev), parts.to(dev)
    ist, fst, fac, hist, ehist = _control_state(N, steps, dev)
    for norm in ("linf", "l2"):
        snaps = []
        for _ in range(2):
            ist[K.FMN_I["k"]].zero_()
            for k in range(steps):
                K.fmn_control(f[k], parts[k], PER, ist, fst, fac, hist, ehist, alpha, gamma, worst, norm)
            K.fmn_control(f[steps], parts[steps], PER, ist, fst, fac, hist, ehist, alpha, gamma, worst, norm, closing=True)
            snaps.append([t.clone() for t in (ist, fst, fac, hist, ehist)])
        for a, b in zip(*snaps):
            assert _same(a.cpu().numpy(), b.cpu().numpy())
        assert int(snaps[0][0][K.FMN_I["found"]].sum()) > 0


# ---- 3. ud_fmn_update: bitwise -----------------------------------------------------------------------------------------------
def _update_case(N, per, seed):
    gen = torch.Generator().manual_seed(seed)
    x0 = torch.rand(N, per, generator=gen) * 2 - 1
    x = (x0 + (torch.rand(N, per, generator=gen) * 2 - 1) * 0.1).clamp(LO, HI)
    x_best = (x0 + (torch.rand(N, per, generator=gen) * 2 - 1) * 0.1).clamp(LO, HI)
    g = torch.randn(N, per, generator=gen)
    g.reshape(-1)[::7] = 0.0
    improved = [n & 1 for n in range(N)]
    eps = [(INF, 0.0, 0.05, 0.5, 0.0123)[n % 5] for n in range(N)]            # rows with eps = +inf and eps = 0 among them
    fac = [(0.7, 0.01, 1e-4, 123.0)[n % 4] for n in range(N)]
    return x, x_best, x0, g, improved, eps, fac


def _update_state(improved, eps, fac, dev):
    from unidefense_amd import kernels as K
    N = len(improved)
    ist, fst = K.fmn_state(N, dev)
    ist[K.FMN_I["improved"]] = torch.tensor(improved, dtype=torch.int32, device=dev)
    fst[K.FMN_F["eps"]] = torch.tensor(eps, dtype=torch.float32, device=dev)
    fst[K.FMN_F["best"]].fill_(NAN)                                        # never read by the update
    return ist, fst, torch.tensor(fac, dtype=torch.float64, device=dev)


def ref_update(x, x_best, x0, g, improved, eps, fac, norm):
    """the same torch expression: z from float64 (product, difference, one rounding to fp32), then fp32 min / max / clamp"""
    imp = torch.tensor(improved).bool().reshape(-1, 1)
    z = (x.double() - g.double() * torch.tensor(fac, dtype=torch.float64).reshape(-1, 1)).float()
    if norm == "linf":
        e = torch.tensor(eps, dtype=torch.float32).reshape(-1, 1)
        z = torch.clamp(torch.min(torch.max(z, x0 - e), x0 + e), LO, HI)
    return z, torch.where(imp, x, x_best)


@pytest.mark.parametrize("N,per", [(1, 1), (1, 3), (8, 5), (3, 27075), (8, 4099), (5, 3 * 64 * 64)])
def test_update_bitwise_vs_torch(N, per):
    from unidefense_amd import kernels as K
    dev = _dev()
    for off in (range(5) if N < 5 else (0,)):
        x, x_best, x0, g, improved, eps, fac = _update_case(N, per, per % 1000 + N)
        improved, eps = [(i + off) & 1 for i in improved], eps[off % len(eps):] + eps[:off % len(eps)]
        if N == 1:
            eps = [(INF, 0.0, 0.05, 0.5, 0.0123)[off]]
        ist, fst, facd = _update_state(improved, eps, fac, dev)
        for norm in ("linf", "l2"):
            want_x, want_best = ref_update(x, x_best, x0, g, improved, eps, fac, norm)
            xd, xbd = x.clone().to(dev), x_best.clone().to(dev)
            K.fmn_update(xd, xbd, x0.to(dev), g.to(dev), ist, fst, facd, norm, LO, HI)
            assert torch.equal(xd.cpu(), want_x), (N, per, off, norm, int((xd.cpu() != want_x).sum()))
            assert torch.equal(xbd.cpu(), want_best), (N, per, off, norm)
            for n in range(N):
                if norm == "linf" and eps[n] == 0.0:
                    assert torch.equal(xd[n].cpu(), x0[n].clamp(LO, HI))
                if norm == "linf" and eps[n] == INF:                     # an infinite budget projects nothing: the clip only
                    z = (x[n].double() - g[n].double() * fac[n]).float()
                    assert torch.equal(xd[n].cpu(), z.clamp(LO, HI))


def test_update_keeps_a_nan_gradient_visible():
    from unidefense_amd import kernels as K
    dev = _dev()
    N, per = 8, 4099
    x, x_best, x0, g, improved, eps, fac = _update_case(N, per, 9)
    bad = [0, 6, 4095, 4098, 4099, 2 * 4099 + 1, 5 * 4099 + 17]            # rows 0 (eps inf), 1 (eps 0), 2, 5 (eps inf)
    g.reshape(-1)[bad] = NAN
    ist, fst, facd = _update_state(improved, eps, fac, dev)
    for norm in ("linf", "l2"):
        want_x, want_best = ref_update(x, x_best, x0, g, improved, eps, fac, norm)     # torch's min / max / clamp keep a NaN
        xd, xbd = x.clone().to(dev), x_best.clone().to(dev)
        K.fmn_update(xd, xbd, x0.to(dev), g.to(dev), ist, fst, facd, norm, LO, HI)
        got = xd.cpu().reshape(-1)
        assert torch.isnan(got[bad]).all() and int(torch.isnan(got).sum()) == len(bad)
        keep = torch.ones(N * per, dtype=torch.bool)
        keep[bad] = False
        assert torch.equal(got[keep], want_x.reshape(-1)[keep]) and torch.equal(xbd.cpu(), want_best)


# ---- 4. ud_fmn_project_l2 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,per", [(3, 5), (4, 4099), (4, 3 * 64 * 64)])
def test_project_l2_is_attack_project_l2_with_a_budget_per_sample(N, per):
    """one ball element for both entry points: with the same finite eps in every row ud_fmn_project_l2 gives the bits of
    ud_attack_project_l2; with a budget per row, row n is the row of ud_attack_project_l2 at eps[n]; eps = inf leaves the clip
    only.  Row 0 lies inside the ball (factor exactly 1), the others outside; one element of row 2 is NaN and stays NaN."""
    from unidefense_amd import kernels as K
    dev = _dev()
    eps = 0.5
    gen = torch.Generator().manual_seed(N * per)
    x0 = torch.rand(N, per, generator=gen) * 2 - 1
    d = torch.rand(N, per, generator=gen) * 2 - 1
    d = d / d.norm(dim=1, keepdim=True) * eps * torch.tensor([0.5] + [3.0] * (N - 1)).reshape(-1, 1)
    x = (x0 + d).to(dev)
    x0d = x0.to(dev)
    dss = K.sample_sumsq(x, x0d)
    x[2, per // 2] = NAN                                   # after the norms: dss is an input of both entry points
    _, fst = K.fmn_state(N, dev)
    fst[K.FMN_F["eps"]].fill_(eps)
    want = K.attack_project_l2(x.clone(), x0d, dss, eps, LO, HI)
    got = K.fmn_project_l2(x.clone(), x0d, dss, fst, LO, HI)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(got[0], x[0].clamp(LO, HI)) and not torch.equal(got[1], x[1])
    assert bool(torch.isnan(got[2, per // 2])) and int(torch.isnan(got).sum()) == 1
    row_eps = [(0.25, INF, 1.0, 0.0)[n % 4] for n in range(N)]
    fst[K.FMN_F["eps"]] = torch.tensor(row_eps, device=dev)
    got = K.fmn_project_l2(x.clone(), x0d, dss, fst, LO, HI)
    for n in range(N):
        if row_eps[n] == INF:
            assert torch.equal(got[n].view(torch.int32), x[n].clamp(LO, HI).view(torch.int32))
        else:
            w = K.attack_project_l2(x.clone(), x0d, dss, row_eps[n], LO, HI)
            assert torch.equal(got[n].view(torch.int32), w[n].view(torch.int32)), n
        if row_eps[n] == 0.0:
            assert torch.equal(got[n], x0d[n].clamp(LO, HI))


# ---- 5. the runner: exact properties -----------------------------------------------------------------------------------------
def _norms(xa, x, norm):
    d = xa.cpu() - x.cpu()
    return d.abs().flatten(1).amax(1) if norm == "linf" else d.double().flatten(1).norm(dim=1)


@pytest.mark.parametrize("norm", ["linf", "l2"])
@pytest.mark.parametrize("name,size,n,seed,steps", [("UDR18", 128, 2, 5, 1), ("UDR18", 128, 2, 5, 3), ("UDR18", 128, 2, 5, 10),
                                                    ("UDEB4", 256, 2, 7, 3)])
def test_fmn_runner_exact_properties(name, size, n, seed, steps, norm):
    from unidefense_amd.attack import FMNRunner
    dev = _dev()
    m = _shared(name, dev)
    x = param_fill.make_input(n, size, seed).to(dev)
    y = param_fill.make_labels(n).to(dev)
    assert float(x.min()) >= LO and float(x.max()) <= HI
    r = FMNRunner(m, n, size, norm=norm, steps=steps)
    assert r.args["method"] == "fmn" and r.args["steps"] == steps and r.args["norm"] == norm
    assert r.args["alpha_final"] == 0.01 and r.args["objective"] == "margin"
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
    assert tuple(radius.shape) == tuple(found.shape) == tuple(margin0.shape) == (n,) and found.dtype == torch.int32
    assert tuple(hist.shape) == (steps + 1, n) and tuple(ehist.shape) == (steps, n) and torch.equal(margin0, hist[0])
    assert tuple(r.g.shape) == tuple(x.shape) and set(r.out) == {"cls_out", "rec", "loss_dict"}
    print(f"  FMN {name} {norm} steps {steps}: radius {radius.tolist()}  found {found.tolist()}  margin0 {margin0.tolist()}")
    print(f"    history {[[round(float(v), 5) for v in row] for row in hist]}")
    print(f"    eps_history {[[round(float(v), 5) for v in row] for row in ehist]}")
    assert torch.isfinite(hist).all()
    for out in (warm, xa):
        assert torch.isfinite(out).all() and float(out.min()) >= LO and float(out.max()) <= HI
    assert torch.equal(found.bool(), torch.isfinite(radius))
    got = _norms(xa, x, norm)
    for i in range(n):
        if found[i]:
            if norm == "linf":
                assert float(radius[i]) == float(got[i]), (i, float(radius[i]), float(got[i]))
            else:
                rel = abs(float(radius[i]) - float(got[i])) / max(float(got[i]), 1e-300) if float(got[i]) > 0 else float(radius[i])
                assert within(f"FMNRunner {name} l2 steps {steps}: radius vs |x_adv - x|_2 in float64, rel", rel, 1e-6)
        else:
            assert torch.equal(xa[i], x[i])                              # nothing found: the input, untouched
        if float(margin0[i]) < 0:                                       # misclassified as it is: radius 0, the clamped input
            assert found[i] and float(radius[i]) == 0.0 and torch.equal(xa[i], x[i].clamp(LO, HI))
    if name == "UDR18":
        # the float64 oracle gives margin0 -2.67 and +3.45 on this fixture: sample 0 is misclassified as it is
        assert [bool(v < 0) for v in margin0] == [True, False], margin0
    within(f"FMNRunner {name} {norm} steps {steps}: replay vs eager warm-up x_adv, max|d| (recorded)",
           float((xa - warm).abs().max()), 2.0)


@pytest.mark.parametrize("name,size,n,seed,norm,steps,precision",
                         [("UDR18", 128, 2, 5, "linf", 10, "fp32"), ("UDR18", 128, 2, 5, "l2", 10, "fp32"),
                          ("UDEB4", 256, 2, 7, "linf", 6, "fp32"), ("UDEB4", 256, 2, 7, "linf", 6, "fp16")])
def test_objective_at_x_adv_is_the_one_its_best_was_set_at(name, size, n, seed, norm, steps, precision):
    """The runner keeps no f of its best point, so the test records, in the eager first call, the iteration at which `improved`
    last fired for each sample (the closing evaluation is iteration `steps`).  The objective that the same-precision forward
    gives at x_adv (the eager eval forward for fp32, the fp16 InferenceRunner for fp16) is THAT row of history, held as
    tests/test_l_apgd_gpu.py::test_best_loss_is_the_loss_at_x_adv holds APGD's best_loss: within 1e-5 — relative to max|cls_out|,
    since an objective on the decision boundary is a difference of logits that nearly cancel — and that row is negative.  The
    UDEB4 cases are the effect test's (section 6): sample 0 is flipped at a distance, in fp32 and in half storage."""
    from unidefense_amd.attack import FMNRunner
    from unidefense_amd.infer import InferenceRunner
    dev = _dev()
    m = _shared(name, dev)
    x = param_fill.make_input(n, size, seed).to(dev)
    y = param_fill.make_labels(n).to(dev)
    kw = _fixture(name)[1]
    r = FMNRunner(m, n, size, norm=norm, steps=steps, precision=precision, **kw)
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
    assert bool(found.all()) and bool((r.radius > 0).any())          # every sample found, at least one at a distance
    for i in range(n):
        assert bool(fired[:, i].any())
        k = int(fired[:, i].nonzero().max())
        d = abs(float(hist[k, i]) - float(mg[i]))
        print(f"  FMN {name} {norm} {precision} sample {i}: best set at k = {k}, objective(x_adv) {float(mg[i]):.6g}, history[{k}] "
              f"{float(hist[k, i]):.6g}, |d| / max|cls_out| {d / scale:.2e}, radius {float(r.radius[i]):.6g}")
        assert float(hist[k, i]) < 0
        assert within(f"FMNRunner {name} {norm} {precision}: objective of the forward at x_adv vs history at the iteration that set "
                      f"best, |d| / max|cls_out|", d / scale, 1e-5)
    xb = r(x, y)                                           # the capture and the first replay: the same attack
    assert r.graph is not None
    within(f"FMNRunner {name} {norm} {precision}: replay vs eager x_adv, max|d| (recorded)", float((xb - xa).abs().max()), 2.0)


def test_fmn_runner_call_refusals_targeted_and_callable_objective():
    from unidefense_amd.attack import FMNRunner, margin_each
    dev = _dev()
    m = _shared("UDR18", dev)
    x = param_fill.make_input(2, 128, 5).to(dev)
    y = param_fill.make_labels(2).to(dev)
    r = FMNRunner(m, 2, 128, steps=1)
    with pytest.raises(ValueError, match="cuda"):
        r(x.cpu(), y)
    with pytest.raises(ValueError, match="differs"):
        r(x[:1], y)
    with pytest.raises(ValueError, match="differ"):
        r(x, y.int())
    assert r.calls == 0
    flags = [p.requires_grad for p in m.parameters()]
    bad = FMNRunner(m, 2, 128, steps=1, objective=lambda out, yy: out["cls_out"].sum())
    with pytest.raises(ValueError, match="one value per sample"):
        bad(x, y)
    assert [p.requires_grad for p in m.parameters()] == flags
    # targeted towards 1 - y is the untargeted attack of a two-class model: -margin(out, 1 - y) = margin(out, y), the same bits
    plain = FMNRunner(m, 2, 128, steps=3)
    plain(x, y)
    a = plain(x, y).clone()
    tgt = FMNRunner(m, 2, 128, steps=3, targeted=True)
    tgt(x, 1 - y)
    assert torch.equal(tgt(x, 1 - y), a) and torch.equal(tgt.radius, plain.radius) and torch.equal(tgt.history, plain.history)

    def margin(out, yy):
        return margin_each(out, yy)
    call = FMNRunner(m, 2, 128, steps=3, objective=margin)
    assert call.args["objective"] == "margin"
    call(x, y)
    assert torch.equal(call(x, y), a)


# ---- 6. effect, judged by the oracle -----------------------------------------------------------------------------------------
# ref_fmn run entirely in the float64 oracle (margin_each on the oracle's forward), checked on the CPU first:
#   UDR18 128^2 n=2 seed 5, steps 10: found both; radii 0 and 0.01503 (linf), 0 and 1.8437 (l2); margin0 -2.67 / +3.45
#   UDEB4 256^2 n=2 seed 7: margin0 +0.9414 / -0.9432, and the param-filled UDEB4 is almost flat in its input: with the plain
#     margin the reference never flips sample 0 (alpha_init 1: 0.9414 -> 0.9361 in 5 steps with eps at its cap, the whole clip
#     box; alpha_init 256, most elements on a clip bound: 0.9227).  So the UDEB4 cases ask for the radius at a CONFIDENCE
#     threshold — objective margin - 0.9394 (_eb4_objective; f0 = +0.00201 / -1.8826) — with alpha_init 32, so that the
#     L2-normalised step fills the linf box in 196 608 dimensions (alpha_init 1 leaves 0.0003 of f0 uncrossed after 5 steps).
#     linf, steps 6: the reference finds both samples, radii 0.038240 and 0; sample 0 is adversarial at k = 4, 5 and at the
#     closing point (f = -5.4e-5, -1.2e-4, -1.3e-4), eps 0.02237, 0.03337, 0.03817, 0.03892, 0.03840, 0.03824.
#     (threshold 0.9374, f0 = 0.004, steps 6: radius 0.11233, but found at the closing point only, at f = -1.4e-4: not used)
EB4_SHIFT, EB4_ALPHA = 0.9394, 32.0
EFFECT = [("UDR18", 128, 2, 5, "linf", 10, "fp32"), ("UDR18", 128, 2, 5, "l2", 10, "fp32"),
          ("UDEB4", 256, 2, 7, "linf", 6, "fp32"), ("UDEB4", 256, 2, 7, "linf", 6, "fp16")]
RATIO_BAR = (1.0 + GAMMA0) / (1.0 - GAMMA0) - 1.0          # one flipped decision's worth of eps: 0.105


def _eb4_objective(out, y):
    """the margin above a confidence threshold: negative once the true class leads by less than EB4_SHIFT"""
    from unidefense_amd.attack import margin_each
    return margin_each(out, y) - EB4_SHIFT


def _fixture(name):
    """(shift of the margin, FMNRunner keywords) of a model's effect cases"""
    return (EB4_SHIFT, dict(alpha_init=EB4_ALPHA, objective=_eb4_objective)) if name == "UDEB4" else (0.0, {})


def _margin64(name, x64, y):
    from unidefense_amd.attack import margin_each
    return margin_each(_oracle_fwd(name, x64), y) - _fixture(name)[0]


@functools.lru_cache(maxsize=None)
def _oracle_fmn(name, size, n, seed, norm, steps):
    x = param_fill.make_input(n, size, seed)
    y = param_fill.make_labels(n)

    def fg(x64, need_grad):
        if not need_grad:
            with torch.no_grad():
                return _margin64(name, x64, y), None
        xg = x64.detach().clone().requires_grad_()
        f = _margin64(name, xg, y)
        g, = torch.autograd.grad(f.sum(), xg)
        return f.detach(), g
    return ref_fmn(fg, x, norm, steps, alpha_init=_fixture(name)[1].get("alpha_init", 1.0), lo=LO, hi=HI)


@pytest.mark.parametrize("name,size,n,seed,norm,steps,precision", EFFECT)
def test_fmn_effect_judged_by_the_oracle(name, size, n, seed, norm, steps, precision):
    """On the samples the GPU found, the ORACLE's objective at the GPU's x_adv is at most 1e-3 max|cls_out64| (the best point lies
    on the boundary by construction, so the oracle may see a positive value no larger than the suite's plain output bound; fp16:
    the yardstick of tests/test_k_attack_fp16_gpu.py — four times the distance of the oracle on fp16-rounded parameters and
    input from the oracle, no less than 5e-3); the GPU finds every sample the reference finds; radius_gpu / radius_ref - 1 <=
    (1 + gamma0) / (1 - gamma0) - 1.  The reference finds every sample of every case; its radii, observed on the CPU: UDR18 0 and
    0.01503 (linf), 0 and 1.8437 (l2); UDEB4 (margin - 0.9394, alpha_init 32, linf, steps 6) 0.038240 and 0.  Observed on the
    GPU: DESIGN 3o."""
    from unidefense_amd.attack import FMNRunner
    dev = _dev()
    m = _shared(name, dev)
    x = param_fill.make_input(n, size, seed)
    y = param_fill.make_labels(n)
    r = FMNRunner(m, n, size, norm=norm, steps=steps, precision=precision, **_fixture(name)[1])
    r(x.to(dev), y.to(dev))
    xa = r(x.to(dev), y.to(dev)).cpu()
    radius, found = r.radius.cpu().double(), r.found.cpu().bool()
    ref = _oracle_fmn(name, size, n, seed, norm, steps)
    with torch.no_grad():
        out64 = _oracle_fwd(name, xa.double())
        m64 = _margin64(name, xa.double(), y)
        scale = float(out64["cls_out"].abs().max())
        clean64 = _oracle_fwd(name, x.double())["cls_out"]
    print(f"  FMN {name} {precision} {norm} steps {steps}: radius gpu {radius.tolist()}  ref {ref['radius'].tolist()}  found gpu "
          f"{found.tolist()} ref {ref['found']}")
    print(f"    f64(x_adv) {m64.tolist()}  max|cls_out64| {scale:.4g}  f0 gpu {r.margin0.tolist()} ref {ref['history'][0]}")
    print(f"    oracle eps_history {[[round(v, 6) for v in row] for row in ref['eps_history']]}")
    print(f"    gpu eps_history    {[[round(float(v), 6) for v in row] for row in r.eps_history]}")
    print(f"    oracle history {[[round(v, 6) for v in row] for row in ref['history']]}")
    print(f"    gpu history    {[[round(float(v), 6) for v in row] for row in r.history]}")
    if precision == "fp32":
        bar = 1e-3                                        # the suite's plain bound
    else:
        from tests.test_k_attack_fp16_gpu import _states
        sd, sd16 = _states()
        with torch.no_grad():
            c16 = eb4.forward_eb4(sd16, x.half().double(), training=False)["cls_out"]
        bar = max(4.0 * float((c16 - clean64).abs().max() / clean64.abs().max()), 5e-3)
    assert ref["found"] == [1] * n                        # the fixture's premise: the reference finds every sample
    assert any(float(v) > 0 for v in ref["radius"])       # and at least one of them at a distance
    ok = []
    for i in range(n):
        assert bool(found[i]), (i, "the reference found this sample, the GPU did not")
        rr = float(ref["radius"][i])
        ratio = float(radius[i]) / rr - 1.0 if rr > 0 else (0.0 if float(radius[i]) == 0.0 else INF)
        ok.append(within(f"FMN effect {name} {precision} {norm} steps {steps}: radius_gpu / radius_ref - 1", ratio, RATIO_BAR))
        ok.append(within(f"FMN effect {name} {precision} {norm} steps {steps}: oracle objective at x_adv / (bar max|cls_out64|)",
                         float(m64[i]) / (bar * scale), 1.0))
    assert all(ok), (radius, ref["radius"], m64, scale, bar)


# ---- 7. what the runner leaves alone -----------------------------------------------------------------------------------------
def test_fmn_leaves_the_model_and_the_other_runners_as_they_were():
    from unidefense_amd import lib
    from unidefense_amd.attack import APGDRunner, AttackRunner, FMNRunner
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
    apgd = APGDRunner(m, n, 256, norm="l2", eps=0.5, steps=2)
    before = []
    for r in (pgd, apgd):
        r(x, y)
        before.append(r(x, y).clone())
        assert r.graph is not None
    caches = {k: dict(m.__dict__.get(k, {})) for k in ("_ud_runners", "_ud_grad_runners", "_ud_attack_runners", "_ud_apgd_runners",
                                                        "_ud_square_runners")}
    path = lib.call("ud_gemm_get_path")
    for r in (FMNRunner(m, n, 256, norm="linf", steps=3), FMNRunner(m, n, 256, norm="l2", steps=3), m.fmn_runner(n, 256, steps=2)):
        for _ in range(3):
            r(x, y)
    torch.cuda.synchronize()
    assert lib.call("ud_gemm_get_path") == path
    assert len(m.__dict__["_ud_fmn_runners"]) == 1
    assert {k: dict(m.__dict__.get(k, {})) for k in caches} == caches
    assert [p.requires_grad for p in m.parameters()] == flags
    assert all(p.grad is None for p in m.parameters())
    assert not m.training
    now = dict(m.named_buffers())
    assert all(torch.equal(v, now[k]) for k, v in bufs.items())
    assert torch.equal(pgd(x, y), before[0]) and torch.equal(apgd(x, y), before[1])     # captured before: the same bits
    got = _train_grads(m, x, y, dev)
    assert got.keys() == want.keys() and len(got) > 300
    diff = [k for k in got if not torch.equal(got[k], want[k])]
    assert not diff, diff[:10]


def test_captured_fmn_runner_follows_an_optimizer_step():
    from unidefense_amd.attack import FMNRunner
    dev = _dev()
    n = 2
    m = _build("UDEB4", dev).eval()
    x = param_fill.make_input(n, 256, 51).to(dev)
    y = param_fill.make_labels(n).to(dev)
    at = FMNRunner(m, n, 256, norm="linf", steps=2)
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
    at2 = FMNRunner(m, n, 256, norm="linf", steps=2)
    at2(x, y)
    assert torch.equal(a1, at2(x, y)) and torch.equal(h1, at2.history) and _same(r1.cpu().numpy(), at2.radius.cpu().numpy())


# ---- 8. the engine -----------------------------------------------------------------------------------------------------------
def test_engine_test_robust_fmn():
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
    attack = {"method": "fmn", "norm": "linf", "steps": 5, "eps": 0.0}
    eng.test_robust(batches=2, attack=attack)                                   # the eager warm-up and the capture
    res = eng.test_robust(batches=2, attack=attack)
    assert attack == {"method": "fmn", "norm": "linf", "steps": 5, "eps": 0.0}   # the caller's dict is not consumed
    assert set(res) == {"clean", "adv", "attack"}
    runner_args = eng.model_without_ddp.fmn_runner(res["clean"]["scores"].numel() // 2, 128, norm="linf", steps=5).args
    assert set(res["attack"]) == set(runner_args) | {"eps", "radius", "found", "median_radius"}
    assert {k: res["attack"][k] for k in runner_args} == runner_args and res["attack"]["method"] == "fmn"
    assert res["attack"]["eps"] == 0.0 and res["attack"]["steps"] == 5 and res["attack"]["gamma_init"] == 0.05
    _same_result(res["clean"], t0)
    radius, found = res["attack"]["radius"], res["attack"]["found"]
    ns = res["clean"]["scores"].numel()
    assert not radius.is_cuda and not found.is_cuda and tuple(radius.shape) == tuple(found.shape) == (ns,)
    assert torch.equal(found.bool(), torch.isfinite(radius))
    assert res["attack"]["median_radius"] == float(radius.double().median())
    # eps = 0: only a sample that is adversarial as it is (radius 0: x_adv = clamp(x) = x) is taken — the clean scores, bitwise
    assert torch.equal(res["adv"]["scores"], res["clean"]["scores"])
    assert torch.equal(res["adv"]["labels"], res["clean"]["labels"])
    # eps absent: every found sample is scored at its adversarial point
    free = eng.test_robust(batches=2, attack={"method": "fmn", "norm": "linf", "steps": 5})
    assert free["attack"]["eps"] is None and _same(free["attack"]["radius"].numpy(), radius.numpy())
    _same_result(free["clean"], t0)
    clean, adv = _mean_ce(free["clean"]), _mean_ce(free["adv"])
    print(f"  radius {radius.tolist()}  found {found.tolist()}  mean cross-entropy of the scores: clean {clean:.4f}  adv {adv:.4f}")
    assert bool(found.any()) and adv >= clean
    # the curve from this one run
    med = res["attack"]["median_radius"]
    curve = robust_curve(radius, [0.0, med])
    assert float(curve[0]) == float((radius > 0).double().mean()) and float(curve[1]) == float((radius > med).double().mean())
    assert float(curve[0]) <= 1.0 - float((found.bool() & (radius == 0)).double().mean()) and float(curve[1]) <= float(curve[0])
    assert float(curve[1]) >= float((~found.bool()).double().mean())             # a sample never found is robust at every eps
    with pytest.raises(ValueError, match="fmn"):
        eng.test_robust(batches=1, attack={"method": "cw", "eps": 0.1})
    with pytest.raises(ValueError, match="eps"):
        eng.test_robust(batches=1, attack={"method": "fmn", "eps": -1.0})
    _same_result(eng.test(batches=2), t0)
    assert all(p.grad is None for p in eng.model_without_ddp.parameters())
