"""CPU: Auto-PGD (unidefense_amd/attack.py: APGDRunner; csrc/apgd.hip) — the checkpoint table, what the runner and the entry
points refuse before any GPU work, the accessor's cache — and the restatement of the algorithm that tests/test_l_apgd_gpu.py
compares the kernels and the runner against: ref_apgd_control (pure Python, the per-sample state machine), ref_update_linf (the
torch fp32 expression, operation by operation), the float64 L2 pieces and ref_apgd (the whole attack in float64 on any
objective that gives per-sample values and a gradient)."""
import ctypes
import math

import pytest
import torch

from tests.test_attack_cpu import ref_project_l2, ref_sample_sumsq

UD_EINVAL = -1000
MODELS = ("UDEB4", "UDR18", "UDR50")


# ---- the definition, restated ------------------------------------------------------------------------------------------------
def ref_checkpoints(steps):
    """p_0 = 0, p_1 = 22, p_{j+1} = p_j + max(p_j - p_{j-1} - 3, 6) hundredths of steps; w_j = ceil(p_j steps / 100) in integers,
    deduplicated, those in [1, steps - 1]"""
    ps = [0, 22]
    while ps[-1] < 100:
        ps.append(ps[-1] + max(ps[-1] - ps[-2] - 3, 6))
    ws = []
    for p in ps[1:]:
        w = (p * steps + 99) // 100
        if 1 <= w <= steps - 1 and w not in ws:
            ws.append(w)
    return tuple(ws)


class ref_apgd_control:
    """The per-sample state machine of one restart, in pure Python on Python floats (an fp32 value is exactly a Python float,
    and halving is exact in both, so on fp32 inputs every array equals the kernel's).  step(f) consumes f_k for k = 0, 1, ...
    and returns the lists (improved, reset, a, eta) that the update of iteration k obeys; close(f) is the closing evaluation."""

    def __init__(self, N, steps, rho, alpha, eta0):
        self.N, self.steps, self.rho, self.alpha = N, steps, rho, alpha
        ws = ref_checkpoints(steps)
        self.window = {w: w - (ws[j - 1] if j else 0) for j, w in enumerate(ws)}
        self.k = 0
        self.f_prev, self.f_best, self.f_ckpt = [0.0] * N, [0.0] * N, [0.0] * N
        self.eta = [eta0] * N
        self.cnt, self.halved = [0] * N, [0] * N
        self.improved, self.reset, self.a = [0] * N, [0] * N, [0.0] * N
        self.history = [[0.0] * N for _ in range(steps + 1)]

    def step(self, f):
        k = self.k
        assert 0 <= k < self.steps
        for n in range(self.N):
            fk = f[n]
            if k == 0:
                self.f_best[n] = self.f_ckpt[n] = fk
                self.improved[n], self.cnt[n], self.halved[n], self.a[n] = 1, 0, 0, 1.0
            else:
                self.cnt[n] += 1 if fk > self.f_prev[n] else 0
                self.improved[n] = 1 if fk > self.f_best[n] else 0
                if self.improved[n]:
                    self.f_best[n] = fk
                self.a[n] = self.alpha
            self.reset[n] = 0
            if k in self.window:
                c1 = self.cnt[n] < self.rho * self.window[k]
                c2 = (not self.halved[n]) and self.f_ckpt[n] == self.f_best[n]
                if c1 or c2:
                    self.eta[n] = self.eta[n] / 2
                    self.reset[n], self.halved[n], self.a[n] = 1, 1, 1.0
                else:
                    self.halved[n] = 0
                self.f_ckpt[n] = self.f_best[n]
                self.cnt[n] = 0
            self.f_prev[n] = fk
            self.history[k][n] = fk
        self.k = k + 1
        return list(self.improved), list(self.reset), list(self.a), list(self.eta)

    def close(self, f):
        for n in range(self.N):
            self.improved[n] = 1 if f[n] > self.f_best[n] else 0
            if self.improved[n]:
                self.f_best[n] = f[n]
            self.history[self.steps][n] = f[n]
        return list(self.improved)


def _ps(v, like):
    """a per-sample list as a column that broadcasts over `like` [N, ...]"""
    return torch.tensor(v, dtype=like.dtype).reshape(-1, *([1] * (like.dim() - 1)))


def ref_update_linf(x, x_prev, x_best, g_best, x0, g, improved, reset, eta, a, eps, lo, hi):
    """The L-infinity update in the dtype of the inputs, one torch operation (one rounding) per arithmetic operation, in the
    order csrc/apgd.hip evaluates it.  Returns (x, x_prev, x_best, g_best) afterwards.  NaN in g is the caller's case:
    torch.sign(NaN) is 0, the kernel keeps the NaN."""
    imp, rst = _ps(improved, x).bool(), _ps(reset, x).bool()
    eta, a = _ps(eta, x), _ps(a, x)
    x_best = torch.where(imp, x, x_best)
    g_best = torch.where(imp, g, g_best)
    src = torch.where(rst, x_best, x)
    gs = torch.where(rst, g_best, g)

    def P(v):
        return torch.clamp(torch.min(torch.max(v, x0 - eps), x0 + eps), lo, hi)
    z = P(src + eta * torch.sign(gs))
    t1 = a * (z - src)
    t2 = (1 - a) * (src - x_prev)
    w = P((src + t1) + t2)
    return torch.where(a == 1, z, w), src, x_best, g_best


def ref_step_l2_apgd(x, x_best, g_best, gss_best, g, improved, reset, eta):
    """float64: (src, z_raw, increment, x_best, g_best, gss_best) of the L2 step — keep-best, source selection and
    z_raw = src + eta gs / max(|gs|_2, 1e-12)"""
    x, x_best, g_best, g = x.double(), x_best.double(), g_best.double(), g.double()
    imp, rst = _ps(improved, x).bool(), _ps(reset, x).bool()
    gss = ref_sample_sumsq(g)
    x_best, g_best = torch.where(imp, x, x_best), torch.where(imp, g, g_best)
    gss_best = torch.where(imp.reshape(-1), gss, gss_best.double())
    src, gs = torch.where(rst, x_best, x), torch.where(rst, g_best, g)
    ss = torch.where(rst.reshape(-1), gss_best, gss)
    inc = gs * (_ps(eta, x) / torch.sqrt(ss).clamp_min(1e-12).reshape(-1, *([1] * (x.dim() - 1))))
    return src, src + inc, inc, x_best, g_best, gss_best


def ref_combine(src, z, x_prev, a):
    """float64: (w, momentum increment) with w = z where a == 1 else src + a (z - src) + (1 - a)(src - x_prev)"""
    src, z, x_prev = src.double(), z.double(), x_prev.double()
    a = _ps(a, src)
    inc = a * (z - src) + (1 - a) * (src - x_prev)
    return torch.where(a == 1, z, src + inc), inc


def ref_apgd(fg, x, norm, eps, steps, rho=0.75, alpha=0.75, lo=-1.0, hi=1.0, start=None):
    """One restart of the attack in float64.  fg(x64, need_grad) -> (f [N] float64, gradient of sum f like x or None): the
    per-sample objective that is ASCENDED.  Returns {"x_best", "f_best", "eta", "history" [steps + 1][N], "halved_at": the
    iterations at which some sample's step was halved}."""
    x0 = x.double()
    N = x0.shape[0]
    xk = x0.clamp(lo, hi) if start is None else start.double().clone()
    x_prev = xk.clone()
    x_best, g_best = torch.zeros_like(xk), torch.zeros_like(xk)
    ctl = ref_apgd_control(N, steps, rho, alpha, 2.0 * eps)
    halved_at = []

    def P(v):
        if norm == "linf":
            return torch.clamp(torch.min(torch.max(v, x0 - eps), x0 + eps), lo, hi)
        return ref_project_l2(v, x0, eps, lo, hi)[0]
    for k in range(steps):
        f, g = fg(xk, True)
        improved, reset, a, eta = ctl.step(f.tolist())
        if any(reset):
            halved_at.append(k)
        imp, rst = _ps(improved, xk).bool(), _ps(reset, xk).bool()
        x_best, g_best = torch.where(imp, xk, x_best), torch.where(imp, g.double(), g_best)
        src, gs = torch.where(rst, x_best, xk), torch.where(rst, g_best, g.double())
        if norm == "linf":
            d = torch.sign(gs)
        else:
            d = gs / _ps(torch.sqrt(ref_sample_sumsq(gs)).clamp_min(1e-12).tolist(), gs)
        z = P(src + _ps(eta, xk) * d)
        w, _ = ref_combine(src, z, x_prev, a)
        xk = torch.where(_ps(a, xk) == 1, z, P(w))
        x_prev = src
    f, _ = fg(xk, False)
    x_best = torch.where(_ps(ctl.close(f.tolist()), xk).bool(), xk, x_best)
    return {"x_best": x_best, "f_best": torch.tensor(ctl.f_best, dtype=torch.float64), "eta": list(ctl.eta),
            "history": [list(r) for r in ctl.history], "halved_at": halved_at}


# ---- the checkpoint table ----------------------------------------------------------------------------------------------------
def test_checkpoints():
    from unidefense_amd.attack import apgd_checkpoints, apgd_table
    assert apgd_checkpoints(10) == (3, 5, 6, 7, 8, 9)
    assert apgd_checkpoints(100) == (22, 41, 57, 70, 80, 87, 93, 99)
    assert apgd_checkpoints(5) == (2, 3, 4)
    assert apgd_checkpoints(1) == ()
    for steps in list(range(1, 130)) + [500, 1000, 4096]:
        ws = apgd_checkpoints(steps)
        assert ws == ref_checkpoints(steps), steps
        assert len(ws) <= 16 and all(1 <= w <= steps - 1 for w in ws) and list(ws) == sorted(set(ws))
    # the threshold is the integer form of cnt < rho * window
    for steps, rho in ((10, 0.75), (100, 0.75), (100, 0.7), (37, 1.0), (50, 0.01)):
        ws, thr = apgd_table(steps, rho)
        assert ws == apgd_checkpoints(steps) and len(thr) == len(ws)
        for j, w in enumerate(ws):
            L = w - (ws[j - 1] if j else 0)
            for cnt in range(L + 2):
                assert (cnt < thr[j]) == (cnt < rho * L), (steps, rho, w, cnt)


def test_reference_control_on_hand_sequences():
    """steps 5: checkpoints (2, 3, 4), windows 2, 1, 1"""
    # rising: f rose in every iteration of every window; no halving
    c = ref_apgd_control(1, 5, 0.75, 0.75, 0.5)
    for k, f in enumerate((1.0, 2.0, 3.0, 4.0, 5.0)):
        improved, reset, a, eta = c.step([f])
        assert (improved, reset, eta) == ([1], [0], [0.5]) and a == [1.0 if k == 0 else 0.75]
    assert c.f_best == [5.0] and c.close([4.0]) == [0] and c.close([6.0]) == [1] and c.f_best == [6.0]
    # falling: condition 1 at every checkpoint; the step is halved three times and every halving is a reset with a = 1
    c = ref_apgd_control(1, 5, 0.75, 0.75, 0.5)
    got = [c.step([f]) for f in (5.0, 4.0, 3.0, 2.0, 1.0)]
    assert [g[1] for g in got] == [[0], [0], [1], [1], [1]]
    assert [g[3] for g in got] == [[0.5], [0.5], [0.25], [0.125], [0.0625]]
    assert [g[2] for g in got] == [[1.0], [0.75], [1.0], [1.0], [1.0]]
    assert c.f_best == [5.0] and [g[0] for g in got] == [[1], [0], [0], [0], [0]]
    # plateau with exact ties: a tie is neither a rise nor an improvement
    c = ref_apgd_control(1, 5, 0.75, 0.75, 0.5)
    got = [c.step([2.0]) for _ in range(5)]
    assert [g[1] for g in got] == [[0], [0], [1], [1], [1]] and [g[0] for g in got] == [[1], [0], [0], [0], [0]]
    # rho 0.5: one rise in a window of two is enough for condition 1.  Condition 2 — the best value did not move since the last
    # checkpoint and the step was NOT halved there — fires at k = 3 although f rose; at k = 4 the memory of that halving blocks it
    c = ref_apgd_control(1, 5, 0.5, 0.75, 0.5)
    got = [c.step([f]) for f in (1.0, 3.0, 2.0, 2.5, 2.75)]
    assert [g[1] for g in got] == [[0], [0], [0], [1], [0]]
    assert c.halved == [0] and c.eta == [0.25]
    # condition 1 alone at k = 3 (no rise in its window of one); at k = 4 f rose and the step was halved at k = 3: nothing fires
    c = ref_apgd_control(1, 5, 0.5, 0.75, 0.5)
    got = [c.step([f]) for f in (1.0, 3.0, 3.5, 3.25, 3.4)]
    assert [g[1] for g in got] == [[0], [0], [0], [1], [0]]
    # a NaN never improves and stays in the history
    c = ref_apgd_control(2, 5, 0.75, 0.75, 0.5)
    for f in ([1.0, 1.0], [float("nan"), 2.0], [3.0, 3.0], [2.0, 4.0], [5.0, 5.0]):
        c.step(f)
    assert math.isnan(c.history[1][0]) and c.f_best == [5.0, 5.0]


def test_reference_update_on_hand_values():
    x0 = torch.tensor([[0.0, 0.5, -0.5, 0.95]] * 2)
    x = x0.clone()
    g = torch.tensor([[1.0, 0.0, -2.0, 3.0]] * 2)
    zero = torch.zeros_like(x)
    # a = 1: z alone; eps 0.1, eta 0.2: the step leaves the box and is brought back to its face, then to clip
    xn, xp, xb, gb = ref_update_linf(x, x, zero, zero, x0, g, [1, 1], [0, 0], [0.2, 0.05], [1.0, 1.0], 0.1, -1.0, 1.0)
    assert torch.equal(xn[0], torch.tensor([0.1, 0.5, -0.6, 1.0]))
    assert torch.equal(xn[1], x0[1] + torch.tensor([0.05, 0.0, -0.05, 0.05]))
    assert torch.equal(xp, x) and torch.equal(xb, x) and torch.equal(gb, g)
    # reset without improvement: the source is the best point and its gradient
    xb0 = x0 + 0.01
    xn, xp, xb, gb = ref_update_linf(x, x, xb0, -g, x0, g, [0, 0], [1, 0], [0.05, 0.05], [1.0, 1.0], 0.1, -1.0, 1.0)
    assert torch.equal(xp[0], xb0[0]) and torch.equal(xp[1], x[1]) and torch.equal(xb, xb0)
    assert torch.equal(xn[0], (xb0 + 0.05 * torch.sign(-g))[0].clamp(-1.0, 1.0))
    # momentum: x_prev = src gives src + a (z - src)
    xn, _, _, _ = ref_update_linf(x, x, zero, zero, x0, g, [0, 0], [0, 0], [0.04, 0.04], [0.75, 0.5], 0.1, -1.0, 1.0)
    assert torch.allclose(xn[0], x0[0] + 0.03 * torch.sign(g[0]), atol=1e-7)
    assert torch.allclose(xn[1], x0[1] + 0.02 * torch.sign(g[1]), atol=1e-7)


# ---- ref_apgd on an analytic objective ----------------------------------------------------------------------------------------
def _quadratic(t):
    """f[n] = -|x[n] - t[n]|^2 / 2: concave, its maximiser t"""
    def fg(x, need_grad):
        d = x.double() - t
        return -0.5 * (d * d).flatten(1).sum(1), (-d if need_grad else None)
    return fg


@pytest.mark.parametrize("norm", ["linf", "l2"])
def test_ref_apgd_on_a_quadratic(norm):
    gen = torch.Generator().manual_seed(3)
    x = (torch.rand(3, 2, 5, generator=gen) - 0.5).double()
    eps = 0.1
    # the maximiser far outside the budget: the best point is the budget's nearest point, reached by the first step
    t = x + 0.4 * torch.sign(torch.randn(3, 2, 5, generator=gen, dtype=torch.float64))
    r = ref_apgd(_quadratic(t), x, norm, eps, 10)
    if norm == "linf":
        assert torch.allclose(r["x_best"], x + eps * torch.sign(t - x), atol=1e-12)
    else:
        nrm = torch.sqrt(ref_sample_sumsq(r["x_best"], x))
        assert bool((nrm <= eps * (1 + 1e-12)).all()) and bool((nrm > 0.99 * eps).all())
        want = x + eps * (t - x) / torch.sqrt(ref_sample_sumsq(t, x)).reshape(-1, 1, 1)
        assert torch.allclose(r["x_best"], want, atol=1e-6)
    f0, _ = _quadratic(t)(x, False)
    assert bool((r["f_best"] > f0).all()) and r["history"][0] == f0.tolist()
    # the maximiser inside the budget: the first step overshoots, the step size has to be halved to get close
    t = x + 0.01 * torch.sign(torch.randn(3, 2, 5, generator=gen, dtype=torch.float64))
    r = ref_apgd(_quadratic(t), x, norm, eps, 100)
    f0, _ = _quadratic(t)(x, False)
    assert r["halved_at"] and all(e < 2 * eps for e in r["eta"])
    assert bool((r["f_best"] >= f0).all())
    fb, _ = _quadratic(t)(r["x_best"], False)
    assert torch.equal(fb, r["f_best"])                                # f_best is f at x_best
    if norm == "linf":
        assert float((r["x_best"] - x).abs().max()) <= eps
    assert bool((r["f_best"] > 0.5 * f0).all())                        # f <= 0: at least half of the way to the maximum


def test_ref_apgd_zero_budget_and_start():
    x = torch.tensor([[1.2, -0.3, 0.0]], dtype=torch.float64)
    fg = _quadratic(torch.zeros(1, 3, dtype=torch.float64))
    r = ref_apgd(fg, x, "linf", 0.0, 5)
    assert torch.equal(r["x_best"], x.clamp(-1.0, 1.0)) and all(e == 0.0 for e in r["eta"])
    s = torch.tensor([[0.9, -0.2, 0.05]], dtype=torch.float64)
    r = ref_apgd(fg, x, "linf", 0.1, 1, start=s)
    assert r["history"][0] == fg(s, False)[0].tolist()


# ---- entry points: argument checks come before any HIP call ------------------------------------------------------------------
def test_apgd_entry_points_reject_bad_arguments():
    from unidefense_amd import lib
    h = lib.load()
    b = ctypes.c_void_p(16)               # never dereferenced
    ck = (ctypes.c_int * 3)(2, 3, 4)
    th = (ctypes.c_int * 3)(2, 1, 1)

    def control(f=b, ist=b, fst=b, hist=b, N=4, steps=5, w=ck, t=th, n=3, eta0=0.1, alpha=0.75, closing=0):
        return h.ud_apgd_control(f, ist, fst, hist, N, steps, w, t, n, eta0, alpha, closing, None)
    assert control(f=None) == UD_EINVAL and control(ist=None) == UD_EINVAL and control(fst=None) == UD_EINVAL
    assert control(hist=None) == UD_EINVAL and control(N=0) == UD_EINVAL and control(steps=0) == UD_EINVAL
    assert control(n=-1) == UD_EINVAL and control(n=17) == UD_EINVAL and control(w=None) == UD_EINVAL and control(t=None) == UD_EINVAL
    assert control(eta0=-0.1) == UD_EINVAL and control(eta0=float("nan")) == UD_EINVAL
    assert control(alpha=0.0) == UD_EINVAL and control(alpha=1.5) == UD_EINVAL and control(alpha=float("nan")) == UD_EINVAL
    assert control(steps=4) == UD_EINVAL                                             # checkpoint 4 is outside [1, steps - 1]
    assert control(w=(ctypes.c_int * 3)(2, 2, 4)) == UD_EINVAL                       # not strictly rising
    assert control(w=(ctypes.c_int * 3)(0, 2, 4)) == UD_EINVAL
    assert control(t=(ctypes.c_int * 3)(2, -1, 1)) == UD_EINVAL
    assert control(closing=1, f=None) == UD_EINVAL

    def update(ptrs=(b,) * 8, N=2, per=100, eps=0.1, lo=-1.0, hi=1.0):
        return h.ud_apgd_update_linf(*ptrs, N, per, eps, lo, hi, None)
    for i in range(8):
        assert update(ptrs=tuple(None if j == i else b for j in range(8))) == UD_EINVAL
    assert update(N=0) == UD_EINVAL and update(per=0) == UD_EINVAL and update(eps=-0.1) == UD_EINVAL
    assert update(eps=float("nan")) == UD_EINVAL and update(lo=1.0, hi=-1.0) == UD_EINVAL
    assert update(lo=float("nan")) == UD_EINVAL and update(hi=float("nan")) == UD_EINVAL

    assert h.ud_apgd_keep(None, b, b, 2, 100, None) == UD_EINVAL and h.ud_apgd_keep(b, None, b, 2, 100, None) == UD_EINVAL
    assert h.ud_apgd_keep(b, b, None, 2, 100, None) == UD_EINVAL and h.ud_apgd_keep(b, b, b, 0, 100, None) == UD_EINVAL
    assert h.ud_apgd_keep(b, b, b, 2, 0, None) == UD_EINVAL
    for i in range(9):
        assert h.ud_apgd_step_l2(*(None if j == i else b for j in range(9)), 2, 100, None) == UD_EINVAL
    assert h.ud_apgd_step_l2(*(b,) * 9, 0, 100, None) == UD_EINVAL and h.ud_apgd_step_l2(*(b,) * 9, 2, 0, None) == UD_EINVAL
    for i in range(4):
        assert h.ud_apgd_combine_l2(*(None if j == i else b for j in range(4)), 2, 100, None) == UD_EINVAL
        assert h.ud_apgd_project_l2(*(None if j == i else b for j in range(4)), 2, 100, 0.1, -1.0, 1.0, None) == UD_EINVAL
    assert h.ud_apgd_combine_l2(b, b, b, b, 0, 100, None) == UD_EINVAL and h.ud_apgd_combine_l2(b, b, b, b, 2, 0, None) == UD_EINVAL
    assert h.ud_apgd_project_l2(b, b, b, b, 0, 100, 0.1, -1.0, 1.0, None) == UD_EINVAL
    assert h.ud_apgd_project_l2(b, b, b, b, 2, 100, -0.1, -1.0, 1.0, None) == UD_EINVAL
    assert h.ud_apgd_project_l2(b, b, b, b, 2, 100, float("nan"), -1.0, 1.0, None) == UD_EINVAL
    assert h.ud_apgd_project_l2(b, b, b, b, 2, 100, 0.1, 1.0, -1.0, None) == UD_EINVAL


def test_apgd_entry_points_are_declared_exported_and_bound():
    from tests.test_abi_cpu import header
    from unidefense_amd import lib
    names = header().protos
    handle = ctypes.CDLL(lib.LIB_PATH)
    for n in ("ud_apgd_control", "ud_apgd_update_linf", "ud_apgd_keep", "ud_apgd_step_l2", "ud_apgd_combine_l2",
              "ud_apgd_project_l2"):
        assert n in names and n in lib.EXPORTED and hasattr(handle, n), n


# ---- the runner: refusals that need no GPU -----------------------------------------------------------------------------------
def _model(name):
    from unidefense_amd.model import load_model
    kw = dict(extractor="efficientnet-b4") if name == "UDEB4" else {}
    return load_model(name)(num_classes=2, drop_rate=0.5, **kw).eval()


@pytest.fixture(scope="module", params=MODELS)
def model(request):
    return _model(request.param)


@pytest.mark.parametrize("kw,match", [(dict(norm="l1", eps=0.1), "norm"), (dict(norm=None, eps=0.1), "norm"),
                                      (dict(eps=-1e-3), "eps"), (dict(eps=float("nan")), "eps"), (dict(), "eps"),
                                      (dict(eps=0.1, steps=0), "steps"), (dict(eps=0.1, steps=-3), "steps"),
                                      (dict(eps=0.1, steps=2.5), "steps"),
                                      (dict(eps=0.1, restarts=0), "restarts"), (dict(eps=0.1, restarts=-1), "restarts"),
                                      (dict(eps=0.1, restarts=1.5), "restarts"),
                                      (dict(eps=0.1, rho=0.0), "rho"), (dict(eps=0.1, rho=1.01), "rho"),
                                      (dict(eps=0.1, rho=float("nan")), "rho"),
                                      (dict(eps=0.1, alpha=0.0), "alpha"), (dict(eps=0.1, alpha=-0.5), "alpha"),
                                      (dict(eps=0.1, alpha=1.5), "alpha"), (dict(eps=0.1, alpha=float("nan")), "alpha"),
                                      (dict(eps=0.1, clip=(1.0, -1.0)), "clip"), (dict(eps=0.1, clip=(0.0, 0.0)), "clip"),
                                      (dict(eps=0.1, objective="hinge"), "objective")])
def test_apgd_runner_refuses_bad_arguments(model, kw, match):
    from unidefense_amd.attack import APGDRunner, apgd_runner
    for make in (lambda: APGDRunner(model, 2, 64, **kw), lambda: apgd_runner(model, 2, 64, **kw),
                 lambda: model.apgd_runner(2, 64, **kw)):
        with pytest.raises(ValueError, match=match):
            make()
    assert not model.__dict__.get("_ud_apgd_runners")


def test_apgd_runner_allows_what_it_should_and_refuses_the_rest(model):
    """l2 with random_start, rho = alpha = 1 and restarts > 1 get as far as the device check; training mode, a foreign model
    and a CPU model are refused"""
    from unidefense_amd.attack import APGDRunner
    for kw in (dict(norm="l2", eps=0.5, random_start=True), dict(eps=0.1, rho=1.0, alpha=1.0), dict(eps=0.1, restarts=3),
               dict(eps=0.0, steps=1), dict(eps=0.1, objective=lambda out, y: out["cls_out"][:, 0])):
        with pytest.raises(ValueError, match="cuda"):
            APGDRunner(model, 2, 64, **kw)
        with pytest.raises(ValueError, match="cuda"):
            model.apgd_runner(2, 64, **kw)
    model.train()
    try:
        with pytest.raises(ValueError, match="eval"):
            APGDRunner(model, 2, 64, eps=0.01)
    finally:
        model.eval()
    with pytest.raises(ValueError, match="UDEB4 / UDR18 / UDR50"):
        APGDRunner(torch.nn.Linear(2, 2).eval(), 2, 64, eps=0.1)
    assert not model.__dict__.get("_ud_apgd_runners")


def test_apgd_runner_checks_the_precision_before_cuda(model):
    from unidefense_amd.attack import APGDRunner, apgd_runner
    for mk in (lambda **kw: APGDRunner(model, 2, 128, eps=0.01, **kw), lambda **kw: apgd_runner(model, 2, 128, eps=0.01, **kw),
               lambda **kw: model.apgd_runner(2, 128, eps=0.01, **kw)):
        with pytest.raises(ValueError, match="precision must be one of"):
            mk(precision="bf16")
        with pytest.raises(ValueError, match="cuda" if type(model).__name__ == "UniDefenseModelEb4" else type(model).__name__):
            mk(precision="fp16")
        with pytest.raises(ValueError, match="fp32"):
            mk(grad_scale=1024.0)
        with pytest.raises(ValueError, match="cuda"):
            mk(precision="fp32", grad_scale=1)
    if type(model).__name__ == "UniDefenseModelEb4":
        with pytest.raises(ValueError, match="power of two"):
            APGDRunner(model, 2, 128, eps=0.01, precision="fp16", grad_scale=1000.0)


def test_apgd_key():
    from unidefense_amd.attack import apgd_key
    k = apgd_key(2, 256, eps=0.01)
    assert k == (2, 256, "linf", 0.01, 100, 1, False, 0.75, 0.75, False, (-1.0, 1.0), "cross_entropy")
    assert apgd_key(2, 256, eps=0.01, precision="fp32", grad_scale=1) == k
    k16 = apgd_key(2, 256, eps=0.01, precision="fp16")
    assert k16 != k and k16[: len(k)] == k and k16 == apgd_key(2, 256, eps=0.01, precision="fp16", grad_scale=1024.0)
    assert k16 != apgd_key(2, 256, eps=0.01, precision="fp16", grad_scale=4096)
    assert len({apgd_key(2, 256, eps=0.01, **kw) for kw in (dict(), dict(restarts=2), dict(rho=0.5), dict(alpha=0.5),
                                                           dict(steps=10), dict(norm="l2"), dict(random_start=True))}) == 7


class _Stub:
    def __init__(self, model, *args):
        self.args = args


def test_apgd_accessor_cache(monkeypatch):
    """identity per full argument tuple, oldest-first eviction at _MAX_RUNNERS, most recently used last — and the three other
    caches exactly as they were (the runner class is stubbed: building a real one needs a GPU)"""
    from unidefense_amd import attack, infer
    monkeypatch.setattr(attack, "APGDRunner", _Stub)
    m = _model("UDR18")
    s1, s2, s3 = object(), object(), object()
    m.__dict__["_ud_runners"] = {(2, 64): s1}
    m.__dict__["_ud_grad_runners"] = {(2, 64, "cross_entropy"): s2}
    m.__dict__["_ud_attack_runners"] = {"k": s3}
    r = m.apgd_runner(2, 64, eps=0.1)
    assert m.apgd_runner(2, 64, eps=0.1) is r and m.apgd_runner(2, 64, norm="linf", eps=0.1, steps=100, restarts=1) is r
    assert attack.apgd_runner(m, 2, 64, eps=0.1) is r
    assert r.args == (2, 64, "linf", 0.1, 100, 1, False, 0.75, 0.75, False, (-1.0, 1.0), "cross_entropy", "fp32", None)
    others = [m.apgd_runner(2, 64, eps=0.1, steps=3), m.apgd_runner(2, 64, eps=0.2), m.apgd_runner(2, 64, eps=0.1, norm="l2"),
              m.apgd_runner(2, 64, eps=0.1, restarts=2), m.apgd_runner(2, 64, eps=0.1, rho=0.5)]
    assert len({id(o) for o in others + [r]}) == 6
    cache = m.__dict__["_ud_apgd_runners"]
    assert len(cache) == infer._MAX_RUNNERS == 4
    assert m.apgd_runner(2, 64, eps=0.1) is not r                          # r was evicted
    keep = m.apgd_runner(2, 64, eps=0.1, rho=0.5)
    assert keep is others[-1]
    for e in (0.3, 0.4, 0.5):
        m.apgd_runner(2, 64, eps=e)
    assert m.apgd_runner(2, 64, eps=0.1, rho=0.5) is keep
    assert m.__dict__["_ud_runners"] == {(2, 64): s1}
    assert m.__dict__["_ud_grad_runners"] == {(2, 64, "cross_entropy"): s2}
    assert m.__dict__["_ud_attack_runners"] == {"k": s3}
