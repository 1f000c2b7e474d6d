"""CPU: the sparse minimum-norm attack (unidefense_amd/attack.py: SparseFMNRunner; csrc/sfmn.hip) — what the runner and the entry
points refuse before any GPU work, the accessor's cache — and the restatement of the algorithm that
tests/test_o_sparse_fmn_gpu.py compares the kernels and the runner against: ref_sfmn_norm_parts (the four numbers per
4096-element part in float64), ref_sfmn_control (Python floats: the per-sample state machine, operation by operation as
include/unidefense_hip.h states it), ref_project_l1 (sort-based, float64), ref_project_l0 (the (kk + 1)-th largest value, ties
dropped) and ref_sparse_fmn (the whole attack in float64 on any objective that gives per-sample values and a gradient)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests.test_fmn_cpu import _linear, _model, _nanmax, _ps, _Stub, ref_schedule

UD_EINVAL = -1000
MODELS = ("UDEB4", "UDR18", "UDR50")
CHUNK = 4096
GSS, GMAX, DABS, DCNT = 0, 1, 2, 3
INF = float("inf")
NAN = float("nan")
GAMMA0 = 0.05
ONE_DECISION = (1.0 + GAMMA0) / (1.0 - GAMMA0) - 1.0      # one flipped decision's worth of eps: 0.105


# ---- the definition, restated ------------------------------------------------------------------------------------------------
def ref_sfmn_norm_parts(x, x0, g=None):
    """float64 numpy [N, parts, 4]: per 4096-element part of every sample sum g^2, max |g| (keeps a NaN), sum |x - x0| and the
    number of x != x0 (a NaN differs); g None: the g entries are 0"""
    x, x0 = np.asarray(x, dtype=np.float64), np.asarray(x0, dtype=np.float64)
    N = x.shape[0]
    x, x0 = x.reshape(N, -1), x0.reshape(N, -1)
    g = None if g is None else np.asarray(g, dtype=np.float64).reshape(N, -1)
    per = x.shape[1]
    parts = (per + CHUNK - 1) // CHUNK
    out = np.zeros((N, parts, 4))
    for p in range(parts):
        s = slice(p * CHUNK, min(per, (p + 1) * CHUNK))
        out[:, p, DABS] = np.abs(x[:, s] - x0[:, s]).sum(1)
        out[:, p, DCNT] = (x[:, s] != x0[:, s]).sum(1)
        if g is not None:
            out[:, p, GSS] = (g[:, s] * g[:, s]).sum(1)
            out[:, p, GMAX] = np.abs(g[:, s]).max(1)              # np.max propagates a NaN
    return out


class ref_sfmn_control:
    """The per-sample state machine on Python floats (IEEE doubles, one rounding per operation); `store` rounds what the kernel
    keeps in fp32 (np.float32: every array then equals ud_sfmn_control's bit for bit; np.float64: the attack in plain float64).
    step(f, parts) consumes f_k [N] and the norm parts [N, P, 4] of iteration k; close(f, parts) is the closing evaluation.
    width = hi - lo of the clip (the l0 estimate).  branch counts what a step did: "adv", "lost" (found before, not adversarial
    now), "far" (nothing found yet), "capped" (worst was the smaller), "nan" (e was NaN: eps kept), "floored" (l0: max(e, 0)
    raised e)."""

    def __init__(self, N, steps, norm, alpha, gamma, worst, width=2.0, store=np.float32):
        assert norm in ("l1", "l0")
        self.N, self.steps, self.l0, self.width = N, steps, norm == "l0", float(width)
        self.alpha, self.gamma, self.worst = [float(v) for v in alpha], [float(v) for v in gamma], [float(v) for v in worst]
        self.store = store
        self.k = [0] * N
        self.eps, self.best = [0.0] * N, [0.0] * N
        self.found, self.improved = [0] * N, [0] * N
        self.fac = [0.0] * N
        self.history = [[0.0] * N for _ in range(steps + 1)]
        self.eps_history = [[0.0] * N for _ in range(steps)]
        self.branch = {"adv": 0, "lost": 0, "far": 0, "capped": 0, "nan": 0, "floored": 0}

    def r(self, v):
        with np.errstate(over="ignore"):
            return float(self.store(v))

    @staticmethod
    def _floor(v):
        return v if (v != v or v in (INF, -INF)) else float(math.floor(v))

    @staticmethod
    def _ceil(v):
        return v if (v != v or v in (INF, -INF)) else float(math.ceil(v))

    def _fold(self, parts, n, closing):
        gss = gmax = dabs = dcnt = 0.0
        for p in range(parts.shape[1]):
            dabs = dabs + float(parts[n, p, DABS])
            dcnt = dcnt + float(parts[n, p, DCNT])
            if not closing:
                gss = gss + float(parts[n, p, GSS])
                gmax = _nanmax(gmax, float(parts[n, p, GMAX]))
        return gss, gmax, dabs, dcnt

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
            gss, gmax, dabs, dcnt = self._fold(parts, n, False)
            dn = self.r(dcnt if self.l0 else dabs)
            if k == 0:
                self.eps[n] = self.best[n] = INF
                self.found[n] = 0
            adv = self._best(n, fk, dn)
            gm, E = self.gamma[k], self.eps[n]
            if adv:
                t, b = E * (1.0 - gm), self.best[n]
                if self.l0:
                    t, u = self._floor(t), E - 1.0
                    t = u if u < t else t
                e = t if t < b else b
                self.branch["adv"] += 1
            elif self.found[n]:
                e = E * (1.0 + gm)
                if self.l0:
                    e, u = self._floor(e), E + 1.0
                    e = u if u > e else e
                self.branch["lost"] += 1
            else:
                q = 1e-12 if gmax < 1e-12 else gmax
                if self.l0:
                    c = self._ceil(abs(fk) / (self.width * q))
                    c = 1.0 if c < 1.0 else c
                    e = dn + c
                else:
                    e = dn + abs(fk) / q
                self.branch["far"] += 1
            if self.l0 and e < 0.0:
                e = 0.0
                self.branch["floored"] += 1
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
            _, _, dabs, dcnt = self._fold(parts, n, True)
            dn = self.r(dcnt if self.l0 else dabs)
            adv = self._best(n, fk, dn)
            self.found[n] |= 1 if adv else 0
            self.history[self.steps][n] = fk
        return list(self.improved)


def ref_project_l1(z, x0, eps, lo, hi):
    """float64 [N, ...]: z onto the per-sample L1 ball of radius eps[n] around x0 (sum |z - x0| <= eps or an infinite eps:
    nothing), then onto clip.  Sort-based: with u the |z - x0| in descending order and c their running sums, rho = the largest j
    with u_j > (c_j - eps) / j, tau = (c_rho - eps) / rho, x = x0 + sign(d) max(|d| - tau, 0).  eps = 0 gives clamp(x0)."""
    z, x0 = z.double(), x0.double()
    out = torch.empty_like(z)
    for n in range(z.shape[0]):
        d = (z[n] - x0[n]).reshape(-1)
        a, e = d.abs(), float(eps[n])
        if e == INF or float(a.sum()) <= e:
            out[n] = z[n]
            continue
        u = torch.sort(a, descending=True).values
        c = u.cumsum(0)
        j = torch.arange(1, u.numel() + 1, dtype=torch.float64)
        hit = (u > (c - e) / j).nonzero()
        if hit.numel():
            rho = int(hit.max()) + 1
            tau = (float(c[rho - 1]) - e) / rho
        else:                                                     # eps = 0: nothing is above tau = max |d|
            tau = float(u[0])
        out[n] = (x0[n].reshape(-1) + torch.sign(d) * (a - tau).clamp_min(0.0)).reshape(z[n].shape)
    return out.clamp(lo, hi)


def ref_project_l0(z, x0, eps, lo, hi):
    """float64 [N, ...]: with kk = eps[n] read as an integer, an infinite eps or kk >= per keeps z everywhere; else t = the
    (kk + 1)-th largest |z - x0| counting multiplicity, the elements with |z - x0| > t keep z and every other returns to x0 (ties
    at the threshold are all dropped: at most kk survive, no index order enters); then clip.  Returns (x, kept mask)."""
    z, x0 = z.double(), x0.double()
    out = torch.empty_like(z)
    kept = torch.zeros_like(z, dtype=torch.bool)
    for n in range(z.shape[0]):
        a, e = (z[n] - x0[n]).abs().reshape(-1), float(eps[n])
        if e == INF or int(e) >= a.numel():
            keep = torch.ones_like(a, dtype=torch.bool)
        else:
            t = torch.sort(a, descending=True).values[max(int(e), 0)]
            keep = a > t
        kept[n] = keep.reshape(z[n].shape)
        out[n] = torch.where(kept[n], z[n], x0[n])
    return out.clamp(lo, hi), kept


def ref_sfmn_worst(x0, norm, lo, hi):
    far = torch.maximum(x0 - lo, hi - x0).flatten(1)
    return far.sum(1).tolist() if norm == "l1" else [float(far.shape[1])] * far.shape[0]


def ref_sparse_fmn(fg, x, norm, steps, alpha_init=1.0, alpha_final=None, gamma_init=0.05, gamma_final=0.001, lo=-1.0, hi=1.0):
    """The attack in float64.  fg(x64, need_grad) -> (f [N] float64, gradient of sum f like x or None): the per-sample
    objective, adversarial where f < 0.  Returns {"x_adv", "radius" (inf where nothing was found), "found", "history"
    [steps + 1][N], "eps_history" [steps][N], "branch", "best_at" (the iteration that set each sample's best, -1: none)}."""
    x0 = x.double()
    N = x0.shape[0]
    alpha = ref_schedule(steps, alpha_init, alpha_init / 100.0 if alpha_final is None else alpha_final)
    gamma = ref_schedule(steps, gamma_init, gamma_final)
    ctl = ref_sfmn_control(N, steps, norm, alpha, gamma, ref_sfmn_worst(x0, norm, lo, hi), width=hi - lo, store=np.float64)
    xk = x0.clamp(lo, hi)
    x_best = x0.clone()
    best_at = [-1] * N
    for k in range(steps):
        f, g = fg(xk, True)
        g = g.double()
        improved, eps, fac = ctl.step(f.tolist(), ref_sfmn_norm_parts(xk.numpy(), x0.numpy(), g.numpy()))
        x_best = torch.where(_ps(improved, xk).bool(), xk, x_best)
        best_at = [k if i else b for i, b in zip(improved, best_at)]
        z = xk - g * _ps(fac, xk)
        xk = ref_project_l1(z, x0, eps, lo, hi) if norm == "l1" else ref_project_l0(z, x0, eps, lo, hi)[0]
    f, _ = fg(xk, False)
    improved = ctl.close(f.tolist(), ref_sfmn_norm_parts(xk.numpy(), x0.numpy()))
    x_best = torch.where(_ps(improved, xk).bool(), xk, x_best)
    best_at = [steps if i else b for i, b in zip(improved, best_at)]
    return {"x_adv": x_best, "radius": torch.tensor(ctl.best, dtype=torch.float64), "found": list(ctl.found),
            "history": [list(r) for r in ctl.history], "eps_history": [list(r) for r in ctl.eps_history],
            "branch": dict(ctl.branch), "best_at": best_at}


# ---- the state machine on hand sequences -------------------------------------------------------------------------------------
def _part(gss=0.0, gmax=0.0, dabs=0.0, dcnt=0.0):
    return np.array([[[gss, gmax, dabs, dcnt]]])


def _ctl(norm, steps=4, gamma=0.25, worst=64.0, alpha=0.5, width=2.0):
    """constant tables with exactly representable values: every expected number below is exact"""
    return ref_sfmn_control(1, steps, norm, [alpha] * steps, [gamma] * steps, [worst], width=width)


def test_reference_control_l1_on_hand_sequences():
    # far: eps = sum |x - x0| + |f| / max |g| every time; the count entry and sum g^2 do not enter eps; fac = alpha / |g|_2
    c = _ctl("l1")
    for k, (f, dn) in enumerate(((1.0, 0.0), (0.5, 0.25), (0.25, 0.5), (0.125, 0.5))):
        improved, eps, fac = c.step([f], _part(gss=4.0, gmax=0.5, dabs=dn, dcnt=99.0))
        assert improved == [0] and eps == [dn + f / 0.5] and fac == [0.5 / 2.0], k
    assert c.found == [0] and c.best == [INF] and c.close([0.5], _part(dabs=0.5)) == [0] and c.best == [INF]
    assert c.history == [[1.0], [0.5], [0.25], [0.125], [0.5]] and c.eps_history == [[2.0], [1.25], [1.0], [0.75]]
    assert c.branch == {"adv": 0, "lost": 0, "far": 4, "capped": 0, "nan": 0, "floored": 0}
    # adversarial at k = 0: radius 0, eps = min(inf (1 - gamma), 0) = 0
    c = _ctl("l1")
    assert c.step([-1.0], _part(gss=4.0, gmax=1.0)) == ([1], [0.0], [0.25]) and c.best == [0.0] and c.found == [1]
    assert c.step([-1.0], _part(gss=4.0, gmax=1.0, dabs=0.5)) == ([0], [0.0], [0.25]) and c.best == [0.0]
    # found, lost, found again: eps shrinks by (1 - gamma) while adversarial (never above best), grows by (1 + gamma) while not
    c = _ctl("l1")
    assert c.step([1.0], _part(gss=1.0, gmax=0.5))[1] == [2.0]                            # far: 0 + 1 / 0.5
    assert c.step([-1.0], _part(gss=1.0, gmax=0.5, dabs=2.0))[:2] == ([1], [1.5])           # min(2 0.75, best 2)
    assert c.step([0.5], _part(gss=1.0, gmax=0.5, dabs=1.5))[:2] == ([0], [1.875])          # lost: 1.5 1.25
    assert c.step([-0.5], _part(gss=1.0, gmax=0.5, dabs=1.0))[:2] == ([1], [1.0])           # min(1.875 0.75, best 1) = 1
    assert c.step([-0.5], _part(gss=1.0, gmax=0.5, dabs=0.5)) == ([1], [1.0], [0.5])       # past the last iteration: nothing moves
    assert c.best == [1.0] and c.k == [4]
    assert c.close([-0.5], _part(dabs=0.5)) == [1] and c.best == [0.5]
    assert c.branch == {"adv": 2, "lost": 1, "far": 1, "capped": 0, "nan": 0, "floored": 0}
    # capped by worst; rounded to fp32 once; a zero gradient: both denominators are 1e-12
    c = _ctl("l1", worst=float(np.float32(0.1)))
    assert c.step([1.0], _part(gss=1.0, gmax=0.5))[1] == [float(np.float32(0.1))] and c.branch["capped"] == 1
    c = _ctl("l1")
    assert c.step([1.0], _part(gss=1.0, gmax=3.0))[1] == [float(np.float32(1.0 / 3.0))]
    c = _ctl("l1")
    assert c.step([1.0], _part()) == ([0], [64.0], [0.5 / 1e-12])
    # NaN-e: a NaN f before anything was found keeps eps (at k = 0: the initial inf); a NaN max |g| likewise
    c = _ctl("l1")
    c.step([1.0], _part(gss=1.0, gmax=0.5))
    assert c.step([NAN], _part(gss=1.0, gmax=0.5, dabs=0.5))[:2] == ([0], [2.0]) and c.branch["nan"] == 1
    assert c.step([1.0], _part(gss=1.0, gmax=NAN, dabs=0.5))[1] == [2.0] and c.branch["nan"] == 2
    c = _ctl("l1")
    assert c.step([NAN], _part(gss=1.0, gmax=0.5))[1] == [INF]
    # the maximum keeps a NaN whichever part holds it; the parts are added in index order
    c = _ctl("l1")
    two = np.array([[[1.0, 0.25, 0.5, 0.0], [3.0, 0.5, 0.25, 0.0]]])
    assert c.step([1.0], two) == ([0], [0.75 + 1.0 / 0.5], [0.25])


def test_reference_control_l0_on_hand_sequences():
    # far: eps = count + max(1, ceil(|f| / (width max |g|))): the sum entry does not enter
    c = _ctl("l0")
    assert c.step([3.0], _part(gss=4.0, gmax=0.5, dabs=77.0, dcnt=0.0)) == ([0], [3.0], [0.25])      # ceil(3 / (2 0.5)) = 3
    assert c.step([0.25], _part(gss=4.0, gmax=0.5, dcnt=3.0))[1] == [4.0]                            # ceil(0.25) = 1
    assert c.step([2.5], _part(gss=4.0, gmax=0.5, dcnt=4.0))[1] == [7.0]                             # ceil(2.5) = 3
    assert c.step([1e-30], _part(gss=4.0, gmax=0.5, dcnt=7.0))[1] == [8.0]                           # at least one more
    assert c.branch["far"] == 4
    c = _ctl("l0", width=1.0)
    assert c.step([3.0], _part(gss=4.0, gmax=0.5))[1] == [6.0]                                       # the clip's width enters
    # adversarial at k = 0: floor(inf) = inf, inf - 1 = inf, min with best 0: eps 0 — and max(e, 0) has nothing to do
    c = _ctl("l0")
    assert c.step([-1.0], _part(gss=4.0, gmax=1.0)) == ([1], [0.0], [0.25]) and c.branch["floored"] == 0
    # eps - 1 against the shrink factor: gamma = 1/4: E = 20: floor(15) = 15 < 19; E = 3: floor(2.25) = 2 = 3 - 1; E = 2:
    # floor(1.5) = 1 = 2 - 1; E = 1: floor(0.75) = 0 = 1 - 1; best is far above
    for E, want in ((20.0, 15.0), (3.0, 2.0), (2.0, 1.0), (1.0, 0.0)):
        c = _ctl("l0")
        c.step([9.0], _part(gss=1.0, gmax=0.5, dcnt=E - 9.0))                               # far: eps = (E - 9) + 9
        assert c.eps == [E]
        assert c.step([-1.0], _part(gss=1.0, gmax=0.5, dcnt=50.0))[:2] == ([1], [want]), E
    # at gamma = 1/32 (0.05's neighbourhood) E - 1 is the smaller up to E = 32: floor(31 31/32) = 30 = E - 1 ... and at E = 64 the
    # factor wins: floor(62) = 62 < 63
    for E, want in ((8.0, 7.0), (32.0, 31.0), (64.0, 62.0)):
        c = _ctl("l0", gamma=1.0 / 32.0, worst=1000.0)
        c.step([E], _part(gss=1.0, gmax=0.5))
        assert c.eps == [E]
        assert c.step([-1.0], _part(gss=1.0, gmax=0.5, dcnt=500.0))[1] == [want], E
    # never above best: best 4 found at E = 20
    c = _ctl("l0")
    c.step([20.0], _part(gss=1.0, gmax=0.5))
    assert c.step([-1.0], _part(gss=1.0, gmax=0.5, dcnt=4.0))[:2] == ([1], [4.0]) and c.best == [4.0]
    # max(e, 0): adversarial at eps 0 at a distance (best 5): min(floor(0), -1) = -1 -> 0
    c = _ctl("l0")
    c.step([-1.0], _part(gss=1.0, gmax=0.5, dcnt=5.0))                                     # k = 0: eps = min(inf, best 5) = 5
    assert c.eps == [5.0] and c.best == [5.0]
    for want in (3.0, 2.0, 1.0):
        assert c.step([-1.0], _part(gss=1.0, gmax=0.5, dcnt=9.0))[1] == [want]
    c = _ctl("l0", steps=8)
    c.step([-1.0], _part(gss=1.0, gmax=0.5, dcnt=1.0))                                     # eps = 1
    assert c.step([-1.0], _part(gss=1.0, gmax=0.5, dcnt=9.0))[1] == [0.0] and c.branch["floored"] == 0
    assert c.step([-1.0], _part(gss=1.0, gmax=0.5, dcnt=9.0))[1] == [0.0] and c.branch["floored"] == 1     # -1 -> 0
    # lost: max(E + 1, floor(E (1 + gamma))): E = 0 -> 1, 1 -> 2, 2 -> 3, 3 -> 4 (floor(3.75) = 3 < 4), then 4 -> 5 (floor(5) = 5)
    for want in (1.0, 2.0, 3.0, 4.0, 5.0):
        assert c.step([1.0], _part(gss=1.0, gmax=0.5, dcnt=0.0))[1] == [want]
    assert c.branch["lost"] == 5
    c = _ctl("l0", worst=1000.0)
    c.step([-1.0], _part(gss=1.0, gmax=0.5, dcnt=40.0))
    assert c.step([1.0], _part(gss=1.0, gmax=0.5, dcnt=40.0))[1] == [50.0]                           # floor(40 1.25) = 50 > 41
    # capped by worst = per; NaN-e keeps eps
    c = _ctl("l0", worst=5.0)
    assert c.step([100.0], _part(gss=1.0, gmax=0.5))[1] == [5.0] and c.branch["capped"] == 1
    assert c.step([NAN], _part(gss=1.0, gmax=0.5, dcnt=5.0))[1] == [5.0] and c.branch["nan"] == 1
    c = _ctl("l0")
    assert c.step([1.0], _part()) == ([0], [64.0], [0.5 / 1e-12])                                    # a zero gradient: capped
    # every eps of an l0 run is an integer or inf
    c = _ctl("l0")
    assert c.step([NAN], _part(gss=1.0, gmax=0.5))[1] == [INF]
    # the closing form
    c = _ctl("l0")
    c.step([1.0], _part(gss=1.0, gmax=0.5))
    assert c.close([-1.0], _part(dcnt=3.0, dabs=0.1)) == [1] and c.best == [3.0] and c.found == [1]


def test_ref_sfmn_norm_parts_on_hand_values():
    x0 = np.zeros((2, CHUNK + 3))
    x = x0.copy()
    x[0, 0], x[0, 1], x[0, CHUNK], x[1, 5] = 3.0, -0.5, -4.0, NAN
    g = np.zeros_like(x)
    g[0, 1], g[0, 2], g[1, CHUNK + 2] = -2.0, 1.0, 5.0
    p = ref_sfmn_norm_parts(x, x0, g)
    assert p.shape == (2, 2, 4)
    assert p[0].tolist() == [[5.0, 2.0, 3.5, 2.0], [0.0, 0.0, 4.0, 1.0]]
    assert math.isnan(p[1, 0, DABS]) and p[1, 0, DCNT] == 1.0 and p[1, 0, GSS] == 0.0       # a NaN differs; it counts once
    assert p[1, 1].tolist() == [25.0, 5.0, 0.0, 0.0]
    assert ref_sfmn_norm_parts(x, x0)[0].tolist() == [[0.0, 0.0, 3.5, 2.0], [0.0, 0.0, 4.0, 1.0]]
    g[0, 7] = NAN
    assert math.isnan(ref_sfmn_norm_parts(x, x0, g)[0, 0, GMAX])


# ---- the projections on hand values ------------------------------------------------------------------------------------------
def _t(*rows):
    return torch.tensor(rows, dtype=torch.float64)


def test_ref_project_l1_on_hand_values():
    x0 = _t([0.0, 0.0, 0.0, 0.0])
    z = _t([0.5, -0.25, 0.0, 0.125])                                                      # sum |d| = 0.875
    assert torch.equal(ref_project_l1(z, x0, [1.0], -1, 1), z)                            # inside the ball: untouched
    assert torch.equal(ref_project_l1(z, x0, [0.875], -1, 1), z)                          # on it
    assert torch.equal(ref_project_l1(z, x0, [INF], -1, 1), z)
    assert torch.equal(ref_project_l1(z * 4, x0, [INF], -1, 1), _t([1.0, -1.0, 0.0, 0.5]))     # ... but the clip
    assert torch.equal(ref_project_l1(z, x0, [0.0], -1, 1), x0)                           # eps = 0: x0
    assert torch.equal(ref_project_l1(z + 0.5, x0 + 0.5, [0.0], -1, 0.25), _t([0.25] * 4))     # clamp(x0)
    # tau = 0.125: support {0.5, 0.25}: (0.75 - 0.5) / 2
    assert torch.equal(ref_project_l1(z, x0, [0.5], -1, 1), _t([0.375, -0.125, 0.0, 0.0]))
    # tau = 0.25: support {0.5}: (0.5 - 0.25) / 1; the element AT tau becomes 0
    assert torch.equal(ref_project_l1(z, x0, [0.25], -1, 1), _t([0.25, 0.0, 0.0, 0.0]))
    # all-equal magnitudes share the budget; zeros stay
    z = _t([0.5, -0.5, 0.5, -0.5, 0.0])
    assert torch.equal(ref_project_l1(z, z * 0, [1.0], -1, 1), _t([0.25, -0.25, 0.25, -0.25, 0.0]))
    assert torch.equal(ref_project_l1(z * 0, z * 0, [0.0], -1, 1), z * 0)
    # around a base point, a budget per sample, the clip last
    x0 = _t([0.5, -0.5], [0.5, -0.5])
    z = _t([1.5, -0.75], [1.5, -0.75])                                                    # d = (1, -0.25)
    got = ref_project_l1(z, x0, [0.5, 1.0], -1, 1)
    assert torch.equal(got, _t([1.0, -0.5], [1.0, -0.625]))                               # tau 0.5: (1.0, -0.5); tau 0.125: (1.375 -> 1, -0.625)
    r = ref_project_l1(torch.randn(3, 50, dtype=torch.float64, generator=torch.Generator().manual_seed(1)), torch.zeros(3, 50),
                       [0.5, 3.0, 10.0], -9, 9)
    assert torch.allclose(r.abs().sum(1), _t(0.5, 3.0, 10.0).reshape(-1), rtol=0, atol=1e-13)


def test_ref_project_l0_on_hand_values():
    x0 = _t([0.0, 0.0, 0.0, 0.0, 0.0])
    z = _t([0.5, -0.25, 0.0, 0.125, -2.0])
    keep = lambda e: ref_project_l0(z, x0, [e], -1, 1)[1][0].tolist()
    assert keep(0.0) == [False] * 5                                                       # kk = 0 drops everything
    assert keep(1.0) == [False, False, False, False, True]
    assert keep(2.0) == [True, False, False, False, True]
    assert keep(4.0) == [True, True, False, True, True]                                   # kk = per - 1: all above the smallest
    assert keep(5.0) == [True] * 5 and keep(7.0) == [True] * 5 and keep(INF) == [True] * 5     # kk >= per, inf: everything
    assert torch.equal(ref_project_l0(z, x0, [2.0], -1, 1)[0], _t([0.5, 0.0, 0.0, 0.0, -1.0]))     # kept: clamp(z); dropped: x0
    assert torch.equal(ref_project_l0(z, x0, [INF], -1, 1)[0], _t([0.5, -0.25, 0.0, 0.125, -1.0]))
    assert torch.equal(ref_project_l0(z + 2, x0 + 2, [0.0], -1, 1)[0], _t([1.0] * 5))     # clamp(x0)
    # ties at the threshold are all dropped: at most kk survive, whatever their order
    z = _t([0.5, -0.5, 0.5, 0.25, 1.0])
    keep = lambda e: ref_project_l0(z, z * 0, [e], -1, 1)[1][0].tolist()
    assert keep(1.0) == [False, False, False, False, True]
    assert keep(2.0) == keep(3.0) == [False, False, False, False, True]                   # the threshold is 0.5: its three go
    assert keep(4.0) == [True, True, True, False, True]
    assert ref_project_l0(z * 0 + 0.5, z * 0, [3.0], -1, 1)[1].sum() == 0                 # all equal: nothing survives kk < per
    assert ref_project_l0(z * 0, z * 0, [3.0], -1, 1)[1].sum() == 0                       # zeros


# ---- ref_sparse_fmn on closed forms ------------------------------------------------------------------------------------------
def _l0_true(w, x, f0, lo, hi):
    """the smallest k whose k largest |w_i| room_i reach f0: room_i is how far coordinate i can move f down inside the box"""
    out = []
    for n in range(x.shape[0]):
        room = torch.where(w[0] > 0, x[n] - lo, hi - x[n]).reshape(-1) * w.abs().reshape(-1)
        c = torch.sort(room, descending=True).values.cumsum(0)
        out.append(int((c < float(f0[n])).sum()) + 1)
    return out


# measured from the reference alone (the printed lines below): the largest observed radius / closed form - 1, plus one
# decision's worth of eps
L1_BAR = 0.0089 + ONE_DECISION
L0_BAR = 0.0 + ONE_DECISION


@pytest.mark.parametrize("steps", [30, 100])
def test_ref_sparse_fmn_linear_l1(steps):
    """f = <w, x> + b in 768 dimensions, every coordinate with room for it: the minimum L1 radius is f0 / max |w| (all of it on
    the coordinate of the largest |w|).  Observed radius / true - 1 with alpha_init 2: 1.7e-4 .. 8.82e-3 at 30 steps,
    6.9e-6 .. 2.4e-5 at 100.  L1_BAR = 0.0089 (the largest observed, rounded up) plus one decision's worth of eps,
    (1 + gamma0) / (1 - gamma0) - 1 = 0.1053: 0.1142."""
    gen = torch.Generator().manual_seed(7)
    w = torch.randn(1, 3, 16, 16, generator=gen, dtype=torch.float64)
    x = (torch.rand(5, 3, 16, 16, generator=gen, dtype=torch.float64) - 0.5) * 0.02
    fg = _linear(w, 1.0)
    f0, _ = fg(x, False)
    assert bool((f0 > 0).all())
    true = f0 / w.abs().max()
    assert float(true.max()) < 0.8                                 # the box allows it: one coordinate carries the whole radius
    r = ref_sparse_fmn(fg, x, "l1", steps, alpha_init=2.0)
    ratio = r["radius"] / true
    print(f"  ref_sparse_fmn linear l1 steps {steps}: radius / true - 1 {(ratio - 1).tolist()}  branches {r['branch']}")
    assert r["found"] == [1] * 5
    assert bool((ratio >= 1.0 - 1e-12).all()) and bool((ratio - 1.0 <= L1_BAR).all()), ratio
    fa, _ = fg(r["x_adv"], False)
    assert bool((fa < 0).all())
    assert torch.allclose((r["x_adv"] - x).abs().flatten(1).sum(1), r["radius"], rtol=1e-12, atol=0)
    assert r["branch"]["adv"] > 0 and r["branch"]["far"] > 0


@pytest.mark.parametrize("steps", [30, 100])
def test_ref_sparse_fmn_linear_l0(steps):
    """the same objective with a larger offset: the minimum L0 radius is the smallest k whose k largest |w_i| room_i reach f0.
    True radius 11 elements for all five samples; observed with alpha_init 32: 11 for every sample at 30 and at 100 steps
    (ratio - 1 = 0).  L0_BAR = 0 plus one decision's worth of eps, 0.1053: a radius of 12 passes, 13 does not."""
    gen = torch.Generator().manual_seed(7)
    w = torch.randn(1, 3, 16, 16, generator=gen, dtype=torch.float64)
    x = (torch.rand(5, 3, 16, 16, generator=gen, dtype=torch.float64) - 0.5) * 0.02
    fg = _linear(w, 30.0)
    f0, _ = fg(x, False)
    assert bool((f0 > 0).all())
    true = torch.tensor(_l0_true(w, x, f0, -1.0, 1.0), dtype=torch.float64)
    assert float(true.min()) >= 5
    r = ref_sparse_fmn(fg, x, "l0", steps, alpha_init=32.0)
    ratio = r["radius"] / true
    print(f"  ref_sparse_fmn linear l0 steps {steps}: true {true.tolist()} radius {r['radius'].tolist()} ratio - 1 "
          f"{(ratio - 1).tolist()}  branches {r['branch']}")
    assert r["found"] == [1] * 5
    assert bool((ratio >= 1.0).all()) and bool((ratio - 1.0 <= L0_BAR).all()), ratio
    fa, _ = fg(r["x_adv"], False)
    assert bool((fa < 0).all())
    assert torch.equal(((r["x_adv"] - x) != 0).flatten(1).sum(1).double(), r["radius"])
    assert all(float(e) == math.floor(e) or e == INF for row in r["eps_history"] for e in row)
    assert r["branch"]["adv"] > 0 and r["branch"]["far"] > 0


def test_ref_sparse_fmn_clean_misclassified_and_unreachable():
    """a sample that starts adversarial has radius 0 (l1: |clamp(x) - x|_1; l0: the clamped elements) and x_adv = clamp(x); one
    whose boundary lies outside clip is never found: radius inf, x_adv = x (not clamped), eps capped by worst"""
    w = torch.ones(1, 1, 4, dtype=torch.float64)
    x = torch.tensor([[[-0.5, 0.2, 1.25, -0.4]], [[0.5, 0.5, 0.5, 0.5]]], dtype=torch.float64)
    for norm, rad in (("l1", 0.25), ("l0", 1.0)):
        r = ref_sparse_fmn(_linear(w, -1.0), x, norm, 10)            # f = sum(x) - 1: adversarial as it is, and +1
        assert r["found"][0] == 1 and float(r["radius"][0]) == rad and torch.equal(r["x_adv"][0], x[0].clamp(-1.0, 1.0))
        r = ref_sparse_fmn(_linear(w, 10.0), x, norm, 10)            # f >= 6 everywhere in clip
        assert r["found"] == [0, 0] and bool(torch.isinf(r["radius"]).all()) and torch.equal(r["x_adv"], x)
        assert r["branch"]["capped"] > 0
        assert max(r["eps_history"][-1]) <= max(ref_sfmn_worst(x, norm, -1.0, 1.0))
    assert ref_sfmn_worst(x, "l0", -1.0, 1.0) == [4.0, 4.0] and ref_sfmn_worst(x, "l1", -1.0, 1.0) == [1.5 + 1.2 + 2.25 + 1.4, 6.0]


# ---- entry points: argument checks come before any HIP call ------------------------------------------------------------------
def test_sfmn_entry_points_reject_bad_arguments():
    from unidefense_amd import lib
    h = lib.load()
    b = ctypes.c_void_p(16)               # never dereferenced
    N, per = 2, 5000
    need = h.ud_sfmn_norms_ws_bytes(N, per)
    assert need == N * 2 * 4 * 8 and h.ud_sfmn_norms_ws_bytes(1, 1) == 32 and h.ud_sfmn_norms_ws_bytes(3, CHUNK) == 96
    assert h.ud_sfmn_norms_ws_bytes(0, per) == UD_EINVAL and h.ud_sfmn_norms_ws_bytes(N, 0) == UD_EINVAL
    assert h.ud_sfmn_norms_ws_bytes(70000, per) == UD_EINVAL

    def parts(x=b, x0=b, g=b, N=N, per=per, ws=b, ws_bytes=need):
        return h.ud_sfmn_norm_parts(x, x0, g, N, per, ws, ws_bytes, None)
    assert parts(x=None) == UD_EINVAL and parts(x0=None) == UD_EINVAL and parts(ws=None) == UD_EINVAL
    assert parts(N=0) == UD_EINVAL and parts(per=0) == UD_EINVAL and parts(ws_bytes=need - 1) == UD_EINVAL
    assert parts(g=None, ws_bytes=0) == UD_EINVAL and parts(g=None, x=None) == UD_EINVAL

    big = 1 << 24
    need_big = h.ud_sfmn_norms_ws_bytes(1, big)

    def control(ptrs=(b,) * 10, ws_bytes=need, N=N, per=per, steps=5, norm=0, lo=-1.0, hi=1.0, closing=0):
        f, ws, rest = ptrs[0], ptrs[1], ptrs[2:]
        return h.ud_sfmn_control(f, ws, ws_bytes, *rest, N, per, steps, norm, lo, hi, closing, None)
    for i in range(10):
        for closing in (0, 1):
            for norm in (0, 1):
                assert control(ptrs=tuple(None if j == i else b for j in range(10)), closing=closing, norm=norm) == UD_EINVAL, i
    assert control(N=0) == UD_EINVAL and control(per=0) == UD_EINVAL and control(steps=0) == UD_EINVAL
    assert control(norm=2) == UD_EINVAL and control(norm=-1) == UD_EINVAL and control(ws_bytes=need - 8) == UD_EINVAL
    assert control(closing=1, steps=0) == UD_EINVAL
    assert control(lo=1.0, hi=-1.0) == UD_EINVAL and control(lo=0.0, hi=0.0) == UD_EINVAL and control(lo=NAN) == UD_EINVAL
    assert control(hi=NAN) == UD_EINVAL
    assert control(N=1, per=big, norm=1, ws_bytes=need_big) == UD_EINVAL                   # an L0 count must stay exact in fp32

    def select(ptrs=(b,) * 6, N=N, per=per, norm=0):
        return h.ud_sfmn_select(*ptrs, N, per, norm, None)
    for i in range(6):
        for norm in (0, 1):
            assert select(ptrs=tuple(None if j == i else b for j in range(6)), norm=norm) == UD_EINVAL, i
    assert select(N=0) == UD_EINVAL and select(per=0) == UD_EINVAL and select(norm=2) == UD_EINVAL and select(norm=-1) == UD_EINVAL
    assert select(N=70000) == UD_EINVAL and select(N=1, per=big, norm=1) == UD_EINVAL

    def apply(ptrs=(b,) * 7, N=N, per=per, norm=0, lo=-1.0, hi=1.0):
        return h.ud_sfmn_apply(*ptrs, N, per, norm, lo, hi, None)
    for i in range(7):
        for norm in (0, 1):
            assert apply(ptrs=tuple(None if j == i else b for j in range(7)), norm=norm) == UD_EINVAL, i
    assert apply(N=0) == UD_EINVAL and apply(per=0) == UD_EINVAL and apply(norm=3) == UD_EINVAL
    assert apply(lo=1.0, hi=-1.0) == UD_EINVAL and apply(lo=NAN) == UD_EINVAL and apply(hi=NAN) == UD_EINVAL
    # FMN's own entry points still take their two norms only
    assert h.ud_fmn_update(*(b,) * 7, N, per, 3, -1.0, 1.0, None) == UD_EINVAL


def test_sfmn_entry_points_are_declared_exported_and_bound():
    from tests.test_abi_cpu import header
    from unidefense_amd import kernels as K
    from unidefense_amd import lib
    names = header().protos
    handle = ctypes.CDLL(lib.LIB_PATH)
    for n in ("ud_sfmn_norms_ws_bytes", "ud_sfmn_norm_parts", "ud_sfmn_control", "ud_sfmn_select", "ud_sfmn_apply"):
        assert n in names and n in lib.EXPORTED and hasattr(handle, n), n
    for n in ("sfmn_state", "sfmn_ws", "sfmn_norms_ws_bytes", "sfmn_norm_parts", "sfmn_control", "sfmn_select", "sfmn_apply"):
        assert callable(getattr(K, n)), n
    assert K.SFMN_I == {"k": 0, "found": 1, "improved": 2} and K.SFMN_F == {"eps": 0, "best": 1}
    assert K.SFMN_NORM == {"l1": 0, "l0": 1} and K.SFMN_PARTS == {"gss": GSS, "gmax": GMAX, "dabs": DABS, "dcnt": DCNT}
    assert K.SFMN_CHUNK == CHUNK == K.FMN_CHUNK and K.sfmn_norms_ws_bytes(3, 3 * 32 * 32) == 3 * 1 * 32
    assert K.FMN_NORM == {"linf": 0, "l2": 1}                               # the sparse norms are no new values of FMN's
    # the header's constants are the binding's
    const = header().consts
    assert const["UD_SFMN_CHUNK"] == CHUNK and const["UD_SFMN_PARTS"] == 4 and const["UD_SFMN_L0_MAX_PER"] == K.SFMN_L0_MAX_PER == 2 ** 24
    assert {k: const[f"UD_SFMN_I_{k.upper()}"] for k in K.SFMN_I} == K.SFMN_I
    assert {k: const[f"UD_SFMN_F_{k.upper()}"] for k in K.SFMN_F} == K.SFMN_F
    assert {k: const[f"UD_SFMN_P_{k.upper()}"] for k in K.SFMN_PARTS} == K.SFMN_PARTS
    assert {k: const[f"UD_SFMN_{k.upper()}"] for k in K.SFMN_NORM} == K.SFMN_NORM


# ---- the runner: refusals that need no GPU -----------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=MODELS)
def model(request):
    return _model(request.param)


@pytest.mark.parametrize("kw,match", [(dict(norm="linf"), "norm"), (dict(norm="l2"), "norm"), (dict(norm=None), "norm"),
                                      (dict(steps=0), "steps"), (dict(steps=-3), "steps"), (dict(steps=2.5), "steps"),
                                      (dict(alpha_init=0.0), "alpha_init"), (dict(alpha_init=-1.0), "alpha_init"),
                                      (dict(alpha_init=float("nan")), "alpha_init"), (dict(alpha_init=float("inf")), "alpha_init"),
                                      (dict(alpha_final=0.0), "alpha_final"), (dict(alpha_final=float("nan")), "alpha_final"),
                                      (dict(gamma_init=0.0), "gamma_init"), (dict(gamma_init=1.0), "gamma_init"),
                                      (dict(gamma_init=float("nan")), "gamma_init"),
                                      (dict(gamma_final=0.0), "gamma_final"), (dict(gamma_final=1.5), "gamma_final"),
                                      (dict(clip=(1.0, -1.0)), "clip"), (dict(clip=(0.0, 0.0)), "clip"),
                                      (dict(objective="hinge"), "objective"), (dict(objective="cross_entropy"), "objective")])
def test_sparse_fmn_runner_refuses_bad_arguments(model, kw, match):
    from unidefense_amd.attack import SparseFMNRunner, sparse_fmn_runner
    for make in (lambda: SparseFMNRunner(model, 2, 64, **kw), lambda: sparse_fmn_runner(model, 2, 64, **kw),
                 lambda: model.sparse_fmn_runner(2, 64, **kw)):
        with pytest.raises(ValueError, match=match):
            make()
    assert not model.__dict__.get("_ud_sparse_fmn_runners") and not model.__dict__.get("_ud_fmn_runners")


def test_sparse_fmn_runner_refuses_l0_where_the_count_is_not_exact(model):
    """3 size^2 >= 2^24 from size 2365 on: the count would no longer be exact in the fp32 state row.  l1 at that size and l0
    just below it get as far as the device check."""
    from unidefense_amd.attack import SparseFMNRunner
    assert 3 * 2365 ** 2 >= 2 ** 24 > 3 * 2364 ** 2
    for size in (2365, 4096):
        with pytest.raises(ValueError, match="2\\^24"):
            SparseFMNRunner(model, 1, size, norm="l0")
        with pytest.raises(ValueError, match="2\\^24"):
            model.sparse_fmn_runner(1, size, norm="l0")
    with pytest.raises(ValueError, match="cuda"):
        SparseFMNRunner(model, 1, 2365, norm="l1")
    with pytest.raises(ValueError, match="cuda"):
        SparseFMNRunner(model, 1, 2364, norm="l0")


def test_sparse_fmn_runner_allows_what_it_should_and_refuses_the_rest(model):
    """both norms, targeted, a callable objective and explicit schedules get as far as the device check; training mode, a
    foreign model and a CPU model are refused; FMNRunner still refuses the sparse norms"""
    from unidefense_amd.attack import NORMS, SPARSE_NORMS, FMNRunner, SparseFMNRunner
    assert SPARSE_NORMS == ("l1", "l0") and NORMS == ("linf", "l2")
    for kw in (dict(), dict(norm="l0", steps=1), dict(norm="l1"), dict(targeted=True),
               dict(alpha_init=8.0, alpha_final=0.5, gamma_init=0.3), dict(objective=lambda out, y: out["cls_out"][:, 0]),
               dict(gamma_final=0.05, clip=(0.0, 1.0))):
        with pytest.raises(ValueError, match="cuda"):
            SparseFMNRunner(model, 2, 64, **kw)
        with pytest.raises(ValueError, match="cuda"):
            model.sparse_fmn_runner(2, 64, **kw)
    model.train()
    try:
        with pytest.raises(ValueError, match="eval"):
            SparseFMNRunner(model, 2, 64)
    finally:
        model.eval()
    with pytest.raises(ValueError, match="UDEB4 / UDR18 / UDR50"):
        SparseFMNRunner(torch.nn.Linear(2, 2).eval(), 2, 64)
    for norm in ("l1", "l0"):
        with pytest.raises(ValueError, match="norm"):
            FMNRunner(model, 2, 64, norm=norm)
    assert not model.__dict__.get("_ud_sparse_fmn_runners")


def test_sparse_fmn_runner_checks_the_precision_before_cuda(model):
    from unidefense_amd.attack import SparseFMNRunner, sparse_fmn_runner
    for mk in (lambda **kw: SparseFMNRunner(model, 2, 128, **kw), lambda **kw: sparse_fmn_runner(model, 2, 128, **kw),
               lambda **kw: model.sparse_fmn_runner(2, 128, **kw)):
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
            SparseFMNRunner(model, 2, 128, precision="fp16", grad_scale=1000.0)


def test_sparse_fmn_key():
    from unidefense_amd.attack import fmn_key, sparse_fmn_key
    k = sparse_fmn_key(2, 256)
    assert k == (2, 256, "l1", 100, 1.0, None, 0.05, 0.001, False, (-1.0, 1.0), "margin")
    assert sparse_fmn_key(2, 256, precision="fp32", grad_scale=1) == k and sparse_fmn_key(2, 256, "l1", 100) == k
    k16 = sparse_fmn_key(2, 256, precision="fp16")
    assert k16 != k and k16[: len(k)] == k and k16 == sparse_fmn_key(2, 256, precision="fp16", grad_scale=1024.0)
    assert k16 != sparse_fmn_key(2, 256, precision="fp16", grad_scale=4096)
    assert len({sparse_fmn_key(2, 256, **kw) for kw in (dict(), dict(norm="l0"), dict(steps=10), dict(alpha_init=8.0),
                                                        dict(alpha_final=0.1), dict(gamma_init=0.1), dict(gamma_final=0.01),
                                                        dict(targeted=True), dict(clip=(0.0, 1.0)))}) == 9
    assert fmn_key(2, 256) == (2, 256, "linf", 100, 1.0, None, 0.05, 0.001, False, (-1.0, 1.0), "margin")


def test_sparse_fmn_accessor_cache(monkeypatch):
    """identity per full argument tuple, oldest-first eviction at _MAX_RUNNERS, most recently used last — and the six other
    caches, _ud_fmn_runners among them, exactly as they were (the runner class is stubbed: building a real one needs a GPU)"""
    from unidefense_amd import attack, infer
    monkeypatch.setattr(attack, "SparseFMNRunner", _Stub)
    m = _model("UDR18")
    slots = ("_ud_runners", "_ud_grad_runners", "_ud_attack_runners", "_ud_apgd_runners", "_ud_square_runners", "_ud_fmn_runners")
    s = [object() for _ in slots]
    for slot, o in zip(slots, s):
        m.__dict__[slot] = {"k": o}
    r = m.sparse_fmn_runner(2, 64)
    assert m.sparse_fmn_runner(2, 64) is r and m.sparse_fmn_runner(2, 64, norm="l1", steps=100, gamma_init=0.05) is r
    assert attack.sparse_fmn_runner(m, 2, 64) is r
    assert r.args == (2, 64, "l1", 100, 1.0, None, 0.05, 0.001, False, (-1.0, 1.0), "margin", "fp32", None)
    others = [m.sparse_fmn_runner(2, 64, steps=3), m.sparse_fmn_runner(2, 64, norm="l0"), m.sparse_fmn_runner(2, 64, gamma_init=0.1),
              m.sparse_fmn_runner(2, 64, alpha_init=8.0), m.sparse_fmn_runner(2, 64, targeted=True)]
    assert len({id(o) for o in others + [r]}) == 6
    cache = m.__dict__["_ud_sparse_fmn_runners"]
    assert len(cache) == infer._MAX_RUNNERS == 4
    assert m.sparse_fmn_runner(2, 64) is not r                                    # r was evicted
    keep = m.sparse_fmn_runner(2, 64, targeted=True)
    assert keep is others[-1]
    for st in (5, 6, 7):
        m.sparse_fmn_runner(2, 64, steps=st)
    assert m.sparse_fmn_runner(2, 64, targeted=True) is keep
    for slot, o in zip(slots, s):
        assert m.__dict__[slot] == {"k": o}


def test_the_two_minimum_norm_runners_share_their_body():
    from unidefense_amd import attack
    assert attack.FMNRunner.__mro__[1] is attack.SparseFMNRunner.__mro__[1]
    for name in ("_buffers", "_iteration", "_closing", "_start", "__call__"):
        assert name not in vars(attack.FMNRunner) and name not in vars(attack.SparseFMNRunner), name
