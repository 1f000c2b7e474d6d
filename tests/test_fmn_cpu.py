"""CPU: the Fast Minimum-Norm attack (unidefense_amd/attack.py: FMNRunner; csrc/fmn.hip) — the schedules, what the runner and
the entry points refuse before any GPU work, the accessor's cache, robust_curve — and the restatement of the algorithm that
tests/test_n_fmn_gpu.py compares the kernels and the runner against: ref_fmn_control (numpy / Python floats: the per-sample state
machine, operation by operation as include/unidefense_hip.h states it), ref_norm_parts (the four norms per 4096-element part in
float64) and ref_fmn (the whole attack in float64 on any objective that gives per-sample values and a gradient)."""
import ctypes
import math

import numpy as np
import pytest
import torch

UD_EINVAL = -1000
MODELS = ("UDEB4", "UDR18", "UDR50")
CHUNK = 4096
GSS, GABS, DSS, DMAX = 0, 1, 2, 3
INF = float("inf")


# ---- the definition, restated ------------------------------------------------------------------------------------------------
def ref_schedule(steps, v0, v1):
    """float64: v1 + (v0 - v1)(1 + cos(pi k / steps)) / 2, k = 0 .. steps - 1"""
    return [v1 + (v0 - v1) * (1.0 + math.cos(math.pi * k / steps)) / 2.0 for k in range(steps)]


def ref_norm_parts(x, x0, g=None):
    """float64 numpy [N, parts, 4]: per 4096-element part of every sample sum g^2, sum |g|, sum (x - x0)^2, max |x - x0| (the
    maximum keeps a NaN); g None: the g entries are 0"""
    x, x0 = np.asarray(x, dtype=np.float64), np.asarray(x0, dtype=np.float64)
    N = x.shape[0]
    x, x0 = x.reshape(N, -1), x0.reshape(N, -1)
    g = None if g is None else np.asarray(g, dtype=np.float64).reshape(N, -1)
    per = x.shape[1]
    parts = (per + CHUNK - 1) // CHUNK
    out = np.zeros((N, parts, 4))
    for p in range(parts):
        s = slice(p * CHUNK, min(per, (p + 1) * CHUNK))
        d = x[:, s] - x0[:, s]
        out[:, p, DSS] = (d * d).sum(1)
        out[:, p, DMAX] = np.abs(d).max(1)                    # np.max propagates a NaN
        if g is not None:
            out[:, p, GSS] = (g[:, s] * g[:, s]).sum(1)
            out[:, p, GABS] = np.abs(g[:, s]).sum(1)
    return out


def _nanmax(m, v):
    return v if (v != v or v > m) else m


class ref_fmn_control:
    """The per-sample state machine on Python floats (IEEE doubles, one rounding per operation); `store` rounds what the kernel
    keeps in fp32 (np.float32: every array then equals ud_fmn_control's bit for bit; np.float64: the attack in plain float64).
    step(f, parts) consumes f_k [N] and the norm parts [N, P, 4] of iteration k; close(f, parts) is the closing evaluation.
    branch counts what step 2 did: "adv", "lost" (found before, not adversarial now), "far" (nothing found yet), "capped" (worst
    was the smaller), "nan" (e was NaN: eps kept)."""

    def __init__(self, N, steps, norm, alpha, gamma, worst, store=np.float32):
        self.N, self.steps, self.l2 = N, steps, norm == "l2"
        self.alpha, self.gamma, self.worst = [float(v) for v in alpha], [float(v) for v in gamma], [float(v) for v in worst]
        self.store = store
        self.k = [0] * N
        self.eps, self.best = [0.0] * N, [0.0] * N
        self.found, self.improved = [0] * N, [0] * N
        self.fac = [0.0] * N
        self.history = [[0.0] * N for _ in range(steps + 1)]
        self.eps_history = [[0.0] * N for _ in range(steps)]
        self.branch = {"adv": 0, "lost": 0, "far": 0, "capped": 0, "nan": 0}

    def r(self, v):
        with np.errstate(over="ignore"):
            return float(self.store(v))

    def _fold(self, parts, n, closing):
        gss = gabs = dss = dmax = 0.0
        for p in range(parts.shape[1]):
            dss = dss + float(parts[n, p, DSS])
            dmax = _nanmax(dmax, float(parts[n, p, DMAX]))
            if not closing:
                gss = gss + float(parts[n, p, GSS])
                gabs = gabs + float(parts[n, p, GABS])
        return gss, gabs, dss, dmax

    def _best(self, n, fk, dn):
        adv = fk < 0.0
        self.improved[n] = 1 if (adv and dn < self.best[n]) else 0
        if self.improved[n]:
            self.best[n] = dn
        return adv

    def step(self, f, parts):
        parts = np.asarray(parts, dtype=np.float64)
        for n in range(self.N):
            k = self.k[n]
            if not 0 <= k < self.steps:
                continue
            fk = float(f[n])
            gss, gabs, dss, dmax = self._fold(parts, n, False)
            dn = self.r(math.sqrt(dss) if self.l2 else dmax)
            if k == 0:
                self.eps[n] = self.best[n] = INF
                self.found[n] = 0
            adv = self._best(n, fk, dn)
            gm, E = self.gamma[k], self.eps[n]
            if adv:
                t, b = E * (1.0 - gm), self.best[n]
                e = t if t < b else b
                self.branch["adv"] += 1
            elif self.found[n]:
                e = E * (1.0 + gm)
                self.branch["lost"] += 1
            else:
                q = math.sqrt(gss) if self.l2 else gabs
                e = dn + abs(fk) / (1e-12 if q < 1e-12 else q)
                self.branch["far"] += 1
            w = self.worst[n]
            if w < e:
                e = w
                self.branch["capped"] += 1
            if e == e:
                self.eps[n] = self.r(e)
            else:
                self.branch["nan"] += 1
            self.found[n] |= 1 if adv else 0
            s = math.sqrt(gss)
            self.fac[n] = self.alpha[k] / (1e-12 if s < 1e-12 else s)
            self.k[n] = k + 1
            self.history[k][n] = fk
            self.eps_history[k][n] = self.eps[n]
        return list(self.improved), list(self.eps), list(self.fac)

    def close(self, f, parts):
        parts = np.asarray(parts, dtype=np.float64)
        for n in range(self.N):
            fk = float(f[n])
            _, _, dss, dmax = self._fold(parts, n, True)
            dn = self.r(math.sqrt(dss) if self.l2 else dmax)
            adv = self._best(n, fk, dn)
            self.found[n] |= 1 if adv else 0
            self.history[self.steps][n] = fk
        return list(self.improved)


def _ps(v, like):
    """a per-sample list as a column that broadcasts over `like` [N, ...]"""
    return torch.tensor(v, dtype=like.dtype).reshape(-1, *([1] * (like.dim() - 1)))


def ref_project(z, x0, eps, norm, lo, hi):
    """float64: z onto the per-sample eps-ball around x0 (an infinite eps projects nothing), then onto clip"""
    e = _ps(eps, z)
    if norm == "linf":
        z = torch.min(torch.max(z, x0 - e), x0 + e)
    else:
        d = z - x0
        nrm = d.flatten(1).norm(dim=1).clamp_min(1e-12).reshape(e.shape)
        z = torch.where(e / nrm < 1.0, x0 + d * (e / nrm), z)
    return z.clamp(lo, hi)


def ref_worst(x0, norm, lo, hi):
    far = torch.maximum(x0 - lo, hi - x0).flatten(1)
    return (far.amax(1) if norm == "linf" else far.norm(dim=1)).tolist()


def ref_fmn(fg, x, norm, steps, alpha_init=1.0, alpha_final=None, gamma_init=0.05, gamma_final=0.001, lo=-1.0, hi=1.0):
    """The attack in float64.  fg(x64, need_grad) -> (f [N] float64, gradient of sum f like x or None): the per-sample
    objective, adversarial where f < 0.  Returns {"x_adv", "radius" (inf where nothing was found), "found", "history"
    [steps + 1][N], "eps_history" [steps][N], "branch"}."""
    x0 = x.double()
    N = x0.shape[0]
    alpha = ref_schedule(steps, alpha_init, alpha_init / 100.0 if alpha_final is None else alpha_final)
    gamma = ref_schedule(steps, gamma_init, gamma_final)
    ctl = ref_fmn_control(N, steps, norm, alpha, gamma, ref_worst(x0, norm, lo, hi), store=np.float64)
    xk = x0.clamp(lo, hi)
    x_best = x0.clone()
    for _ in range(steps):
        f, g = fg(xk, True)
        g = g.double()
        improved, eps, fac = ctl.step(f.tolist(), ref_norm_parts(xk.numpy(), x0.numpy(), g.numpy()))
        x_best = torch.where(_ps(improved, xk).bool(), xk, x_best)
        xk = ref_project(xk - g * _ps(fac, xk), x0, eps, norm, lo, hi)
    f, _ = fg(xk, False)
    improved = ctl.close(f.tolist(), ref_norm_parts(xk.numpy(), x0.numpy()))
    x_best = torch.where(_ps(improved, xk).bool(), xk, x_best)
    return {"x_adv": x_best, "radius": torch.tensor(ctl.best, dtype=torch.float64), "found": list(ctl.found),
            "history": [list(r) for r in ctl.history], "eps_history": [list(r) for r in ctl.eps_history], "branch": dict(ctl.branch)}


# ---- the schedules -----------------------------------------------------------------------------------------------------------
def test_fmn_schedule():
    from unidefense_amd.attack import fmn_schedule
    for steps in (1, 2, 5, 20, 100, 1000):
        alpha, gamma = fmn_schedule(steps)
        assert alpha.dtype == gamma.dtype == torch.float32 and tuple(alpha.shape) == tuple(gamma.shape) == (steps,)
        assert not alpha.is_cuda
        # end points: k = 0 is the initial value exactly; the last value stays above the final one and, for many steps, near it
        assert float(alpha[0]) == 1.0 and float(gamma[0]) == float(np.float32(0.05))
        assert float(alpha[-1]) >= float(np.float32(0.01)) and float(gamma[-1]) >= float(np.float32(0.001))
        # monotone: the cosine falls on [0, pi)
        assert bool((alpha[1:] <= alpha[:-1]).all()) and bool((gamma[1:] <= gamma[:-1]).all())
        # the float64 formula, rounded once
        assert np.array_equal(alpha.numpy(), np.asarray(ref_schedule(steps, 1.0, 0.01)).astype(np.float32))
        assert np.array_equal(gamma.numpy(), np.asarray(ref_schedule(steps, 0.05, 0.001)).astype(np.float32))
    alpha, gamma = fmn_schedule(1000)
    assert float(alpha[-1]) < 0.0101 and float(gamma[-1]) < 0.00101
    alpha, gamma = fmn_schedule(4, alpha_init=2.0, alpha_final=1.0, gamma_init=0.5, gamma_final=0.25)
    assert alpha.tolist() == [float(np.float32(v)) for v in ref_schedule(4, 2.0, 1.0)] and float(alpha[2]) == 1.5
    assert float(gamma[0]) == 0.5 and float(gamma[2]) == 0.375
    assert fmn_schedule(3, alpha_init=0.5)[0][0] == 0.5 and float(fmn_schedule(1, alpha_init=0.5)[0][0]) == 0.5


# ---- the state machine on hand sequences -------------------------------------------------------------------------------------
def _part(gss=0.0, gabs=0.0, dss=0.0, dmax=0.0):
    return np.array([[[gss, gabs, dss, dmax]]])


def _ctl(steps=4, norm="linf", gamma=0.25, worst=8.0, alpha=0.5):
    """constant tables with exactly representable values: every expected number below is exact"""
    return ref_fmn_control(1, steps, norm, [alpha] * steps, [gamma] * steps, [worst])


def test_reference_control_on_hand_sequences():
    # never adversarial: eps is the linearised distance dn + f / |g|_1 every time; nothing found, radius inf
    c = _ctl()
    for k, (f, dn) in enumerate(((1.0, 0.0), (0.5, 0.25), (0.25, 0.5), (0.125, 0.5))):
        improved, eps, fac = c.step([f], _part(gss=4.0, gabs=4.0, dmax=dn))
        assert improved == [0] and eps == [dn + f / 4.0] and fac == [0.5 / 2.0], k
    assert c.found == [0] and c.best == [INF] and c.close([0.5], _part(dmax=0.5)) == [0] and c.best == [INF]
    assert c.history == [[1.0], [0.5], [0.25], [0.125], [0.5]] and c.eps_history == [[0.25], [0.375], [0.5625], [0.53125]]
    assert c.branch == {"adv": 0, "lost": 0, "far": 4, "capped": 0, "nan": 0}
    # l2 reads the other norms: dn = sqrt(dss), the dual norm is |g|_2
    c = _ctl(norm="l2")
    assert c.step([1.0], _part(gss=4.0, gabs=100.0, dss=0.25, dmax=77.0)) == ([0], [0.5 + 1.0 / 2.0], [0.25])
    # adversarial at k = 0: radius 0 and eps = min(inf (1 - gamma), 0) = 0; later adversarial points at a distance never improve
    c = _ctl()
    assert c.step([-1.0], _part(gss=4.0, gabs=4.0)) == ([1], [0.0], [0.25])
    assert c.best == [0.0] and c.found == [1]
    assert c.step([-1.0], _part(gss=4.0, gabs=4.0, dmax=0.5)) == ([0], [0.0], [0.25]) and c.best == [0.0]
    # found, then lost, then found again: eps shrinks by (1 - gamma) while adversarial (never above best), grows by (1 + gamma)
    # while not
    c = _ctl()
    assert c.step([1.0], _part(gss=1.0, gabs=2.0))[1] == [0.5]                        # far: 0 + 1 / 2
    assert c.step([-1.0], _part(gss=1.0, gabs=2.0, dmax=0.5))[:2] == ([1], [0.375])     # min(0.5 0.75, best 0.5)
    assert c.best == [0.5] and c.found == [1]
    assert c.step([0.5], _part(gss=1.0, gabs=2.0, dmax=0.375))[:2] == ([0], [0.46875])  # lost: 0.375 1.25
    assert c.best == [0.5] and c.found == [1]
    assert c.step([-0.5], _part(gss=1.0, gabs=2.0, dmax=0.25))[:2] == ([1], [0.25])     # min(0.46875 0.75, best 0.25) = 0.25
    assert c.best == [0.25]
    assert c.step([-0.5], _part(gss=1.0, gabs=2.0, dmax=0.125)) == ([1], [0.25], [0.5])  # past the last iteration: nothing moves
    assert c.best == [0.25] and c.k == [4]
    assert c.close([-0.5], _part(dmax=0.125)) == [1] and c.best == [0.125]              # the closing evaluation may still improve
    assert c.close([0.5], _part(dmax=0.0)) == [0] and c.best == [0.125]
    assert c.branch == {"adv": 2, "lost": 1, "far": 1, "capped": 0, "nan": 0}
    # a NaN f is never adversarial; before anything was found e is NaN and eps stays; it stays in the history
    c = _ctl()
    c.step([1.0], _part(gss=1.0, gabs=2.0))
    assert c.step([float("nan")], _part(gss=1.0, gabs=2.0, dmax=0.5))[:2] == ([0], [0.5])
    assert math.isnan(c.history[1][0]) and c.found == [0] and c.branch["nan"] == 1
    c.step([-1.0], _part(gss=1.0, gabs=2.0, dmax=0.5))
    assert c.step([float("nan")], _part(gss=1.0, gabs=2.0, dmax=0.5))[1] == [0.375 * 1.25]   # found: the NaN counts as lost
    # a NaN at k = 0 leaves the initial eps = inf: the update then projects nothing
    c = _ctl()
    assert c.step([float("nan")], _part(gss=1.0, gabs=2.0))[1] == [INF]
    # e capped by worst, and rounded to fp32 once
    c = _ctl(worst=float(np.float32(0.1)))
    assert c.step([1.0], _part(gss=1.0, gabs=2.0))[1] == [float(np.float32(0.1))] and c.branch["capped"] == 1
    c = _ctl()
    assert c.step([1.0], _part(gss=1.0, gabs=3.0))[1] == [float(np.float32(1.0 / 3.0))]
    # a zero gradient: both denominators are 1e-12; e is capped
    c = _ctl()
    assert c.step([1.0], _part()) == ([0], [8.0], [0.5 / 1e-12])
    # the parts of a sample are added in index order; the maximum keeps a NaN whichever part holds it
    c = _ctl()
    two = np.array([[[1.0, 1.0, 0.0, 0.25], [3.0, 3.0, 0.0, 0.125]]])
    assert c.step([1.0], two) == ([0], [0.25 + 1.0 / 4.0], [0.25])
    c = _ctl()
    c.step([-1.0], np.array([[[1.0, 1.0, 0.0, float("nan")], [3.0, 3.0, 0.0, 0.125]]]))
    assert c.improved == [0] and c.best == [INF] and c.found == [1]                    # dn is NaN: never the best


def test_ref_norm_parts_on_hand_values():
    x0 = np.zeros((2, CHUNK + 3))
    x = x0.copy()
    x[0, 0], x[0, CHUNK], x[1, 5] = 3.0, -4.0, float("nan")
    g = np.zeros_like(x)
    g[0, 1], g[1, CHUNK + 2] = -2.0, 5.0
    p = ref_norm_parts(x, x0, g)
    assert p.shape == (2, 2, 4)
    assert p[0].tolist() == [[4.0, 2.0, 9.0, 3.0], [0.0, 0.0, 16.0, 4.0]]
    assert math.isnan(p[1, 0, DSS]) and math.isnan(p[1, 0, DMAX]) and p[1, 0, GSS] == 0.0
    assert p[1, 1].tolist() == [25.0, 5.0, 0.0, 0.0]
    assert ref_norm_parts(x, x0)[0].tolist() == [[0.0, 0.0, 9.0, 3.0], [0.0, 0.0, 16.0, 4.0]]


# ---- ref_fmn on closed forms -------------------------------------------------------------------------------------------------
GAMMA0 = 0.05


def _linear(w, b):
    """f[n] = <w, x[n]> + b: the margin of a linear two-class score; adversarial where negative"""
    def fg(x, need_grad):
        f = (x.double() * w).flatten(1).sum(1) + b
        return f, (w.expand_as(x).clone() if need_grad else None)
    return fg


def _ball(c, r):
    """f[n] = |x[n] - c|^2 - r^2: adversarial inside the ball of radius r around c"""
    def fg(x, need_grad):
        d = x.double() - c
        return (d * d).flatten(1).sum(1) - r * r, (2.0 * d if need_grad else None)
    return fg


@pytest.mark.parametrize("steps", [20, 100])
def test_ref_fmn_linear_linf(steps):
    """true radius margin / |w|_1 in 768 dimensions (in a handful of dimensions the first estimate lands exactly on the linear
    boundary and a sample can sit at f = +1e-17 for ever: DESIGN 3o): observed radius / true 1.0026 .. 1.0036 at 20 steps,
    1.00008 .. 1.00013 at 100"""
    gen = torch.Generator().manual_seed(7)
    w = torch.randn(1, 3, 16, 16, generator=gen, dtype=torch.float64)
    x = (torch.rand(5, 3, 16, 16, generator=gen, dtype=torch.float64) - 0.5) * 0.2
    b = 30.0                                                       # |w|_1 ~ 613: true radii around 0.05
    fg = _linear(w, b)
    f0, _ = fg(x, False)
    assert bool((f0 > 0).all())
    true = f0 / w.abs().sum()
    assert float(true.max()) < 0.5                                 # the box never binds: x - true sign(w) stays inside clip
    r = ref_fmn(fg, x, "linf", steps)
    ratio = r["radius"] / true
    print(f"  ref_fmn linear linf steps {steps}: radius / true {ratio.tolist()}  branches {r['branch']}")
    assert r["found"] == [1] * 5
    assert bool((ratio >= 1.0).all()) and bool((ratio <= 1.0 + 2.0 * GAMMA0).all()), ratio
    fa, _ = fg(r["x_adv"], False)
    assert bool((fa < 0).all())
    assert torch.equal((r["x_adv"] - x).abs().flatten(1).amax(1), r["radius"])
    assert r["branch"]["adv"] > 0 and r["branch"]["lost"] > 0 and r["branch"]["far"] > 0


def test_ref_fmn_ball_l2():
    """true radius |x0 - c| - r: observed radius / true - 1 in {0, 2.2e-16} at 50 steps"""
    gen = torch.Generator().manual_seed(11)
    c = (torch.rand(1, 2, 5, generator=gen, dtype=torch.float64) - 0.5) * 0.4
    x = (torch.rand(5, 2, 5, generator=gen, dtype=torch.float64) - 0.5) * 1.6
    rad = 0.25
    fg = _ball(c, rad)
    f0, _ = fg(x, False)
    assert bool((f0 > 0).all())
    true = (x - c).flatten(1).norm(dim=1) - rad
    r = ref_fmn(fg, x, "l2", 50)
    ratio = r["radius"] / true
    print(f"  ref_fmn ball l2 steps 50: radius / true - 1 {(ratio - 1).tolist()}  branches {r['branch']}")
    assert r["found"] == [1] * 5
    assert bool((ratio >= 1.0).all()) and bool((ratio <= 1.0 + 2.0 * GAMMA0).all()), ratio
    fa, _ = fg(r["x_adv"], False)
    assert bool((fa < 0).all())


def test_ref_fmn_clean_misclassified_and_unreachable():
    """a sample that starts adversarial has radius 0 and x_adv = clamp(x); one whose boundary lies outside clip is never found:
    radius inf, x_adv = x (not clamped), eps capped by worst"""
    w = torch.ones(1, 1, 4, dtype=torch.float64)
    x = torch.tensor([[[-0.5, 0.2, 1.25, -0.4]], [[0.5, 0.5, 0.5, 0.5]]], dtype=torch.float64)
    r = ref_fmn(_linear(w, -1.0), x, "linf", 10)                      # f = sum(x) - 1: -0.45 (clamped: -0.7) and +1
    assert r["found"][0] == 1 and float(r["radius"][0]) == 0.25    # |clamp(x) - x| = 0.25: the start point is the best
    assert torch.equal(r["x_adv"][0], x[0].clamp(-1.0, 1.0))
    r = ref_fmn(_linear(w, 10.0), x, "linf", 10)                     # f >= 6 everywhere in clip
    assert r["found"] == [0, 0] and bool(torch.isinf(r["radius"]).all()) and torch.equal(r["x_adv"], x)
    assert r["branch"]["capped"] > 0
    assert max(r["eps_history"][-1]) <= max(ref_worst(x, "linf", -1.0, 1.0))


# ---- robust_curve ------------------------------------------------------------------------------------------------------------
def test_robust_curve_on_hand_values():
    from unidefense_amd.attack import robust_curve
    radius = torch.tensor([0.0, 0.1, INF, 0.3])
    got = robust_curve(radius, [0.0, 0.1, 0.2, 1.0])
    assert got.dtype == torch.float64 and got.tolist() == [0.75, 0.5, 0.5, 0.25]
    assert robust_curve(radius, torch.tensor([0.05])).tolist() == [0.75]
    assert robust_curve(torch.zeros(3), [0.0]).tolist() == [0.0]             # clean-misclassified: never robust, not even at eps 0
    curve = robust_curve(radius, torch.linspace(0, 1, 11))
    assert bool((curve[1:] <= curve[:-1]).all())


# ---- entry points: argument checks come before any HIP call ------------------------------------------------------------------
def test_fmn_entry_points_reject_bad_arguments():
    from unidefense_amd import lib
    h = lib.load()
    b = ctypes.c_void_p(16)               # never dereferenced
    N, per = 2, 5000
    need = h.ud_fmn_norms_ws_bytes(N, per)
    assert need == N * 2 * 4 * 8 and h.ud_fmn_norms_ws_bytes(1, 1) == 32 and h.ud_fmn_norms_ws_bytes(3, CHUNK) == 96
    assert h.ud_fmn_norms_ws_bytes(0, per) == UD_EINVAL and h.ud_fmn_norms_ws_bytes(N, 0) == UD_EINVAL
    assert h.ud_fmn_norms_ws_bytes(70000, per) == UD_EINVAL

    def parts(x=b, x0=b, g=b, N=N, per=per, ws=b, ws_bytes=need):
        return h.ud_fmn_norm_parts(x, x0, g, N, per, ws, ws_bytes, None)
    assert parts(x=None) == UD_EINVAL and parts(x0=None) == UD_EINVAL and parts(ws=None) == UD_EINVAL
    assert parts(N=0) == UD_EINVAL and parts(per=0) == UD_EINVAL and parts(ws_bytes=need - 1) == UD_EINVAL
    assert parts(g=None, ws_bytes=0) == UD_EINVAL and parts(g=None, x=None) == UD_EINVAL

    def control(ptrs=(b,) * 10, ws_bytes=need, N=N, per=per, steps=5, norm=0, closing=0):
        f, ws, rest = ptrs[0], ptrs[1], ptrs[2:]
        return h.ud_fmn_control(f, ws, ws_bytes, *rest, N, per, steps, norm, closing, None)
    for i in range(10):
        for closing in (0, 1):
            assert control(ptrs=tuple(None if j == i else b for j in range(10)), closing=closing) == UD_EINVAL, i
    assert control(N=0) == UD_EINVAL and control(per=0) == UD_EINVAL and control(steps=0) == UD_EINVAL
    assert control(norm=2) == UD_EINVAL and control(norm=-1) == UD_EINVAL and control(ws_bytes=need - 8) == UD_EINVAL
    assert control(closing=1, steps=0) == UD_EINVAL

    def update(ptrs=(b,) * 7, N=N, per=per, norm=0, lo=-1.0, hi=1.0):
        return h.ud_fmn_update(*ptrs, N, per, norm, lo, hi, None)
    for i in range(7):
        for norm in (0, 1):
            assert update(ptrs=tuple(None if j == i else b for j in range(7)), norm=norm) == UD_EINVAL, i
    assert update(N=0) == UD_EINVAL and update(per=0) == UD_EINVAL and update(norm=3) == UD_EINVAL
    assert update(lo=1.0, hi=-1.0) == UD_EINVAL and update(lo=float("nan")) == UD_EINVAL and update(hi=float("nan")) == UD_EINVAL

    def project(ptrs=(b,) * 4, N=N, per=per, lo=-1.0, hi=1.0):
        return h.ud_fmn_project_l2(*ptrs, N, per, lo, hi, None)
    for i in range(4):
        assert project(ptrs=tuple(None if j == i else b for j in range(4))) == UD_EINVAL, i
    assert project(N=0) == UD_EINVAL and project(per=0) == UD_EINVAL and project(lo=1.0, hi=-1.0) == UD_EINVAL
    assert project(lo=float("nan")) == UD_EINVAL


def test_fmn_entry_points_are_declared_exported_and_bound():
    from tests.test_abi_cpu import header
    from unidefense_amd import kernels as K
    from unidefense_amd import lib
    names = header().protos
    handle = ctypes.CDLL(lib.LIB_PATH)
    for n in ("ud_fmn_norms_ws_bytes", "ud_fmn_norm_parts", "ud_fmn_control", "ud_fmn_update", "ud_fmn_project_l2"):
        assert n in names and n in lib.EXPORTED and hasattr(handle, n), n
    for n in ("fmn_state", "fmn_ws", "fmn_norms_ws_bytes", "fmn_norm_parts", "fmn_control", "fmn_update", "fmn_project_l2"):
        assert callable(getattr(K, n)), n
    assert K.FMN_I == {"k": 0, "found": 1, "improved": 2} and K.FMN_F == {"eps": 0, "best": 1}
    assert K.FMN_NORM == {"linf": 0, "l2": 1} and K.FMN_PARTS == {"gss": GSS, "gabs": GABS, "dss": DSS, "dmax": DMAX}
    assert K.FMN_CHUNK == CHUNK and K.fmn_norms_ws_bytes(3, 3 * 32 * 32) == 3 * 1 * 32
    # the header's constants are the binding's
    const = header().consts
    assert const["UD_FMN_CHUNK"] == CHUNK and const["UD_FMN_PARTS"] == 4
    assert {k: const[f"UD_FMN_I_{k.upper()}"] for k in K.FMN_I} == K.FMN_I
    assert {k: const[f"UD_FMN_F_{k.upper()}"] for k in K.FMN_F} == K.FMN_F
    assert {k: const[f"UD_FMN_P_{k.upper()}"] for k in K.FMN_PARTS} == K.FMN_PARTS
    assert {k: const[f"UD_FMN_{k.upper()}"] for k in K.FMN_NORM} == K.FMN_NORM


# ---- the runner: refusals that need no GPU -----------------------------------------------------------------------------------
def _model(name):
    from unidefense_amd.model import load_model
    kw = dict(extractor="efficientnet-b4") if name == "UDEB4" else {}
    return load_model(name)(num_classes=2, drop_rate=0.5, **kw).eval()


@pytest.fixture(scope="module", params=MODELS)
def model(request):
    return _model(request.param)


@pytest.mark.parametrize("kw,match", [(dict(norm="l1"), "norm"), (dict(norm=None), "norm"), (dict(norm="l0"), "norm"),
                                      (dict(steps=0), "steps"), (dict(steps=-3), "steps"), (dict(steps=2.5), "steps"),
                                      (dict(alpha_init=0.0), "alpha_init"), (dict(alpha_init=-1.0), "alpha_init"),
                                      (dict(alpha_init=float("nan")), "alpha_init"), (dict(alpha_init=float("inf")), "alpha_init"),
                                      (dict(alpha_final=0.0), "alpha_final"), (dict(alpha_final=float("nan")), "alpha_final"),
                                      (dict(gamma_init=0.0), "gamma_init"), (dict(gamma_init=1.0), "gamma_init"),
                                      (dict(gamma_init=float("nan")), "gamma_init"),
                                      (dict(gamma_final=0.0), "gamma_final"), (dict(gamma_final=1.5), "gamma_final"),
                                      (dict(clip=(1.0, -1.0)), "clip"), (dict(clip=(0.0, 0.0)), "clip"),
                                      (dict(objective="hinge"), "objective"), (dict(objective="cross_entropy"), "objective")])
def test_fmn_runner_refuses_bad_arguments(model, kw, match):
    from unidefense_amd.attack import FMNRunner, fmn_runner
    for make in (lambda: FMNRunner(model, 2, 64, **kw), lambda: fmn_runner(model, 2, 64, **kw),
                 lambda: model.fmn_runner(2, 64, **kw)):
        with pytest.raises(ValueError, match=match):
            make()
    assert not model.__dict__.get("_ud_fmn_runners")


def test_fmn_runner_allows_what_it_should_and_refuses_the_rest(model):
    """both norms, targeted, a callable objective and explicit schedules get as far as the device check; training mode, a
    foreign model and a CPU model are refused"""
    from unidefense_amd.attack import FMNRunner
    for kw in (dict(), dict(norm="l2", steps=1), dict(targeted=True), dict(alpha_init=0.5, alpha_final=0.5, gamma_init=0.3),
               dict(objective=lambda out, y: out["cls_out"][:, 0]), dict(gamma_final=0.05, clip=(0.0, 1.0))):
        with pytest.raises(ValueError, match="cuda"):
            FMNRunner(model, 2, 64, **kw)
        with pytest.raises(ValueError, match="cuda"):
            model.fmn_runner(2, 64, **kw)
    model.train()
    try:
        with pytest.raises(ValueError, match="eval"):
            FMNRunner(model, 2, 64)
    finally:
        model.eval()
    with pytest.raises(ValueError, match="UDEB4 / UDR18 / UDR50"):
        FMNRunner(torch.nn.Linear(2, 2).eval(), 2, 64)
    assert not model.__dict__.get("_ud_fmn_runners")


def test_fmn_runner_checks_the_precision_before_cuda(model):
    from unidefense_amd.attack import FMNRunner, fmn_runner
    for mk in (lambda **kw: FMNRunner(model, 2, 128, **kw), lambda **kw: fmn_runner(model, 2, 128, **kw),
               lambda **kw: model.fmn_runner(2, 128, **kw)):
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
            FMNRunner(model, 2, 128, precision="fp16", grad_scale=1000.0)


def test_fmn_key():
    from unidefense_amd.attack import fmn_key
    k = fmn_key(2, 256)
    assert k == (2, 256, "linf", 100, 1.0, None, 0.05, 0.001, False, (-1.0, 1.0), "margin")
    assert fmn_key(2, 256, precision="fp32", grad_scale=1) == k and fmn_key(2, 256, "linf", 100) == k
    k16 = fmn_key(2, 256, precision="fp16")
    assert k16 != k and k16[: len(k)] == k and k16 == fmn_key(2, 256, precision="fp16", grad_scale=1024.0)
    assert k16 != fmn_key(2, 256, precision="fp16", grad_scale=4096)
    assert len({fmn_key(2, 256, **kw) for kw in (dict(), dict(norm="l2"), dict(steps=10), dict(alpha_init=0.5),
                                                 dict(alpha_final=0.1), dict(gamma_init=0.1), dict(gamma_final=0.01),
                                                 dict(targeted=True), dict(clip=(0.0, 1.0)))}) == 9


class _Stub:
    def __init__(self, model, *args):
        self.args = args


def test_fmn_accessor_cache(monkeypatch):
    """identity per full argument tuple, oldest-first eviction at _MAX_RUNNERS, most recently used last — and the four other
    caches exactly as they were (the runner class is stubbed: building a real one needs a GPU)"""
    from unidefense_amd import attack, infer
    monkeypatch.setattr(attack, "FMNRunner", _Stub)
    m = _model("UDR18")
    s = [object() for _ in range(5)]
    slots = ("_ud_runners", "_ud_grad_runners", "_ud_attack_runners", "_ud_apgd_runners", "_ud_square_runners")
    for slot, o in zip(slots, s):
        m.__dict__[slot] = {"k": o}
    r = m.fmn_runner(2, 64)
    assert m.fmn_runner(2, 64) is r and m.fmn_runner(2, 64, norm="linf", steps=100, gamma_init=0.05) is r
    assert attack.fmn_runner(m, 2, 64) is r
    assert r.args == (2, 64, "linf", 100, 1.0, None, 0.05, 0.001, False, (-1.0, 1.0), "margin", "fp32", None)
    others = [m.fmn_runner(2, 64, steps=3), m.fmn_runner(2, 64, norm="l2"), m.fmn_runner(2, 64, gamma_init=0.1),
              m.fmn_runner(2, 64, alpha_init=0.5), m.fmn_runner(2, 64, targeted=True)]
    assert len({id(o) for o in others + [r]}) == 6
    cache = m.__dict__["_ud_fmn_runners"]
    assert len(cache) == infer._MAX_RUNNERS == 4
    assert m.fmn_runner(2, 64) is not r                                    # r was evicted
    keep = m.fmn_runner(2, 64, targeted=True)
    assert keep is others[-1]
    for st in (5, 6, 7):
        m.fmn_runner(2, 64, steps=st)
    assert m.fmn_runner(2, 64, targeted=True) is keep
    for slot, o in zip(slots, s):
        assert m.__dict__[slot] == {"k": o}
