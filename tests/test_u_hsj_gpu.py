"""GPU: the decision-based minimum-norm attack's kernels (csrc/hsj.hip), HSJRunner (unidefense_amd/hsj.py) and
test_robust(attack={"method": "hsj"}).

Kernels: every propose mode bitwise against the numpy restatement (the Gaussian probe against its float64 restatement), idle
rows untouched, position independence bitwise; the estimate bitwise (Linf) and against float64 (L2); the control exactly, mode
by mode, over random bit sequences.  Runner: with a known linear classifier the decisions of a whole attack are the
restatement's row for row in the eager, the capturing and the replaying call; then the life cycle on real forwards, and the
stage."""
import copy
import functools
import math

import numpy as np
import pytest
import torch

from oracle import param_fill
from tests import hsj_case as HC
from tests.margins import within
from tests.test_j_attack_gpu import _dev, _shared
from tests.test_s_smooth_gpu import BIG_ID, KERNEL_CASES, SEED, Z_BAR, _bits, _place
from unidefense_amd import hsj as H
from unidefense_amd.smooth import ref_smooth_unit

pytestmark = pytest.mark.gpu

LO, HI = -1.0, 1.0


def _state(N, seed):
    """a mixed per-sample state on the host: (ist [13, N] int32, fst [8, N] float32) as numpy arrays; live, seeking, idle rows"""
    from unidefense_amd import kernels as K
    I, F = K.HSJ_I, K.HSJ_F
    rng = np.random.default_rng(seed)
    ist, fst = np.zeros((len(I), N), dtype=np.int32), np.zeros((len(F), N), dtype=np.float32)
    kind = np.arange(N) % 4 if N > 1 else np.zeros(1, dtype=np.int64)        # 0, 2: live; 1: seeking; 3: idle
    ist[I["active"]] = kind != 3
    ist[I["has"]] = (kind == 0) | (kind == 2)
    ist[I["moved"]] = kind != 2
    ist[I["stepdone"]] = np.arange(N) % 8 == 2
    ist[I["draw"]] = rng.integers(0, 1000, N)
    fst[F["lo"]] = rng.random(N, dtype=np.float32) * np.float32(0.25)
    fst[F["hi"]] = fst[F["lo"]] + rng.random(N, dtype=np.float32) * np.float32(0.5)
    fst[F["delta"]] = rng.random(N, dtype=np.float32) * np.float32(0.3) + np.float32(1e-3)
    fst[F["xi"]] = rng.random(N, dtype=np.float32) + np.float32(0.1)
    fst[F["invn"]] = rng.random(N, dtype=np.float32) * np.float32(0.1)
    return ist, fst


def _ids(N):
    ids = np.arange(N, dtype=np.int64) * 3 + 1
    ids[N // 2] = BIG_ID
    return ids


def _rows(mode, ist, I):
    active, has = ist[I["active"]] != 0, ist[I["has"]] != 0
    if mode == "copy":
        return np.ones_like(active)
    if mode in ("copy_seek", "noise"):
        return active & ~has
    return active & has & ((ist[I["stepdone"]] == 0) if mode == "step" else True)


def _scalar(mode, norm, ist, fst, per, F):
    if mode == "bisect":
        return np.float32(0.5) * (fst[F["lo"]] + fst[F["hi"]])
    if mode == "settle":
        return fst[F["hi"]]
    if mode == "probe":
        return fst[F["delta"]] * np.float32(1.0 / math.sqrt(per)) if norm == "l2" else fst[F["delta"]]
    if mode == "step":
        return fst[F["xi"]] * fst[F["invn"]] if norm == "l2" else fst[F["xi"]]
    return np.zeros(ist.shape[1], dtype=np.float32)


# ---- 1. ud_hsj_propose ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", H.NORMS)
@pytest.mark.parametrize("N,per,offset", KERNEL_CASES)
def test_propose_every_mode_vs_restatement(N, per, offset, norm):
    """Bitwise, but for the Gaussian probe (L2), which is held to the float64 restatement x + s z64 with the bar
      |s| Z_BAR           Z_BAR = 1e-5 is the smooth tests' bound on |z - z64|; here s = delta / sqrt(D)
      + 2^-24 (1 + |s| 5.77)   one rounding of the sum, whose value is at most |x| + |s| |z| <= 1 + 5.77 |s| before the clamp
    (the product's own rounding, 2^-24 |s| 5.77, is inside the first term's slack)."""
    from unidefense_amd import kernels as K
    dev = _dev()
    I, F = K.HSJ_I, K.HSJ_F
    ist, fst = _state(N, N * 131 + per)
    ids = _ids(N)
    gen = torch.Generator().manual_seed(N * 7 + per)
    a, b = (torch.rand(N, per, generator=gen) * 2 - 1 for _ in range(2))
    istd, fstd, idd = torch.from_numpy(ist).to(dev), torch.from_numpy(fst).to(dev), torch.from_numpy(ids).to(dev)
    ad, bd = _place(a, dev, offset), _place(b, dev, offset)
    an, bn = a.numpy(), b.numpy()
    for mode in K.HSJ_P:
        dst = _place(torch.full((N, per), 9.0), dev, offset)
        got = K.hsj_propose(mode, norm, dst, None if mode == "noise" else ad, bd if mode in ("bisect", "settle", "step") else None,
                            idd, istd, fstd, LO, HI, SEED)
        torch.cuda.synchronize()
        assert got is dst and torch.equal(ad.cpu(), a) and torch.equal(bd.cpu(), b)
        rows = _rows(mode, ist, I)
        g = got.cpu().numpy()
        assert (g[~rows] == 9.0).all(), mode                     # an idle row is not touched
        if not rows.any():
            continue
        s = _scalar(mode, norm, ist, fst, per, F)[rows]
        t = None
        if mode in ("noise", "probe"):
            t = ref_smooth_unit(ids[rows], ist[I["draw"]][rows], per, "gaussian" if (mode, norm) == ("probe", "l2") else "uniform", SEED)
        want = H.ref_hsj_propose(mode, norm, an[rows], bn[rows], s, t, LO, HI, plain=ist[I["moved"]][rows] == 0)
        if want.dtype == np.float64:
            err = float(np.abs(g[rows].astype(np.float64) - want).max())
            smax = float(np.abs(s).max())
            print(f"  gaussian probe N {N} per {per}: max |x_try - restatement64| {err:.3e}  max |s| {smax:.3e}")
            assert within(f"hsj gaussian probe N{N} per{per}", err, smax * Z_BAR + 2.0 ** -24 * (1.0 + 5.77 * smax))
            # and bitwise the fp32 expression on the rounded float64 noise, in all but a vanishing part of the elements
            same = _bits(g[rows]) == _bits(H.ref_hsj_propose(mode, norm, an[rows], None, s, t.astype(np.float32), LO, HI))
            assert float(same.mean()) >= 0.999
        else:
            assert want.dtype == np.float32 and np.array_equal(_bits(g[rows]), _bits(want)), (mode, norm)
            assert float(g[rows].min()) >= LO and float(g[rows].max()) <= HI or mode in ("copy", "copy_seek")


@pytest.mark.parametrize("norm", H.NORMS)
def test_probe_does_not_depend_on_the_row_or_on_n(norm):
    from unidefense_amd import kernels as K
    dev = _dev()
    I, F = K.HSJ_I, K.HSJ_F
    N, per = 5, 192
    ist, fst = _state(N, 3)
    ist[I["active"]], ist[I["has"]] = 1, 1
    ids = np.array([1, 2, BIG_ID, 7, 9], dtype=np.int64)
    x = torch.rand(N, per, generator=torch.Generator().manual_seed(3)) * 2 - 1
    to = lambda t: torch.from_numpy(np.ascontiguousarray(t)).to(dev)          # noqa: E731
    full = K.hsj_propose("probe", norm, torch.empty(N, per, device=dev), x.to(dev), None, to(ids), to(ist), to(fst), LO, HI, SEED).cpu()
    for n in (2, 3):                                             # the sample alone, in an N = 1 launch
        alone = K.hsj_propose("probe", norm, torch.empty(1, per, device=dev), x[n:n + 1].to(dev), None, to(ids[n:n + 1]),
                              to(ist[:, n:n + 1]), to(fst[:, n:n + 1]), LO, HI, SEED).cpu()
        assert np.array_equal(_bits(alone[0]), _bits(full[n]))
    p = np.array([4, 2, 0, 1, 3])                                # another row
    perm = K.hsj_propose("probe", norm, torch.empty(N, per, device=dev), x[torch.from_numpy(p)].to(dev), None, to(ids[p]), to(ist[:, p]), to(fst[:, p]),
                         LO, HI, SEED).cpu()
    assert np.array_equal(_bits(perm), _bits(full[p]))
    off = K.hsj_propose("probe", norm, _place(torch.zeros(N, per), dev, True), _place(x, dev, True), None, to(ids), to(ist), to(fst),
                        LO, HI, SEED)
    assert np.array_equal(_bits(off), _bits(full))               # the scalar path: the same bits
    other = K.hsj_propose("probe", norm, torch.empty(N, per, device=dev), x.to(dev), None, to(ids + 1), to(ist), to(fst), LO, HI, SEED)
    assert float((other.cpu() != full).double().mean()) > 0.9


# ---- 2. ud_hsj_dist -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,per,offset", KERNEL_CASES)
def test_dist_vs_float64(N, per, offset):
    from unidefense_amd import kernels as K
    dev = _dev()
    gen = torch.Generator().manual_seed(N + per)
    a, b = (torch.rand(N, per, generator=gen) * 2 - 1 for _ in range(2))
    ist, _ = _state(N, 1)
    for bb in (b, None):
        nrm = torch.full((2, N), -7.0, dtype=torch.float64, device=dev)
        K.hsj_dist(_place(a, dev, offset), None if bb is None else _place(bb, dev, offset), nrm, torch.from_numpy(ist).to(dev))
        d = a.double().numpy() - (0 if bb is None else bb.double().numpy())
        g = nrm.cpu().numpy()
        act = ist[K.HSJ_I["active"]] != 0
        assert (g[:, ~act] == -7.0).all()                        # an idle sample is skipped
        assert np.array_equal(g[1, act], np.abs(d).max(1)[act])  # the maximum is exact
        assert float(np.abs(g[0, act] / (d * d).sum(1)[act] - 1).max()) <= 1e-13


# ---- 3. ud_hsj_estimate ---------------------------------------------------------------------------------------------------------------
def _phi(B, N, rows, seed):
    """int8 [rows, N]: column n all zeros (n % 3 == 0), all ones (1) or mixed (2) in its first B rows; junk behind them"""
    rng = np.random.default_rng(seed)
    phi = rng.integers(0, 2, (rows, N)).astype(np.int8)
    phi[:B, np.arange(N) % 3 == 0] = 0
    phi[:B, np.arange(N) % 3 == 1] = 1
    return phi


@pytest.mark.parametrize("norm", H.NORMS)
@pytest.mark.parametrize("B", [1, 7, 64, 100, 128])
@pytest.mark.parametrize("N,per,offset", KERNEL_CASES)
def test_estimate_vs_restatement(N, per, offset, B, norm):
    """Linf: the sign of the fp32 sum, bitwise.  L2: held to the float64 sum of w_b z64_b with the bar
      sum_b |w_b| Z_BAR            every direction's |z - z64| <= Z_BAR
      + (B + 1) 2^-24 S, S = sum_b |w_b| |z_b|   the fp32 products and the B adds, each rounding at most half an ulp of a partial
                                   sum that S bounds
    and, as the Gaussian probe has it, bitwise against the fp32 restatement (float64 Box-Muller rounded once, fp32 products and
    adds in ascending b) in at least 99.9 % of the elements: a sum in another order, or a contracted multiply-add, differs in the
    last bit of a good part of them.  B = 128 is phi's row count here (max_probes); all-zero, all-one and mixed columns are in
    every case with N >= 3 (N = 1: all-zero)."""
    from unidefense_amd import kernels as K
    dev = _dev()
    rows, draw0 = 128, 40
    phi, ids = _phi(B, N, rows, B * 11 + N), _ids(N)
    v = _place(torch.full((N, per), 9.0), dev, offset)
    got = K.hsj_estimate(v, torch.from_numpy(phi).to(dev), torch.from_numpy(ids).to(dev), B, draw0, norm, SEED)
    torch.cuda.synchronize()
    g = got.cpu().numpy()
    if norm == "linf":
        want = H.ref_hsj_estimate(phi[:B], ids, draw0, per, norm, SEED)
        assert np.array_equal(_bits(g), _bits(want))
        return
    want = H.ref_hsj_estimate(phi[:B], ids, draw0, per, norm, SEED, exact=True)
    w = np.abs(H._weights(phi[:B]).astype(np.float64))
    S = sum(w[b][:, None] * np.abs(ref_smooth_unit(ids, draw0 + b, per, "gaussian", SEED)) for b in range(B))
    bar = w.sum(0)[:, None] * Z_BAR + (B + 1) * 2.0 ** -24 * S
    worst = float((np.abs(g.astype(np.float64) - want) / bar).max())
    print(f"  l2 estimate N {N} per {per} B {B}: max |v - v64| / bar {worst:.3e}")
    assert within(f"hsj l2 estimate N{N} per{per} B{B} (fraction of the bar)", worst, 1.0)
    same = _bits(g) == _bits(H.ref_hsj_estimate(phi[:B], ids, draw0, per, norm, SEED))
    print(f"    bitwise the fp32 restatement in {float(same.mean()):.6f} of the elements")
    assert int((~same).sum()) <= max(1, same.size // 1000)       # (a small case may hold ONE element whose noise rounds the other way)


def test_estimate_live_rows_4096_probes_and_the_refusal():
    from unidefense_amd import kernels as K
    dev = _dev()
    N, per, B = 3, 75, 4096
    assert B == K.HSJ_MAX_PROBES
    phi, ids = _phi(B, N, B, 5), _ids(N)
    phi[:, 0] = np.random.default_rng(1).integers(0, 2, B)      # a mixed sample with 4096 probes
    ist, _ = _state(N, 2)
    ist[K.HSJ_I["active"]], ist[K.HSJ_I["has"]] = [1, 1, 1], [1, 0, 1]
    v = torch.full((N, per), 9.0, device=dev)
    K.hsj_estimate(v, torch.from_numpy(phi).to(dev), torch.from_numpy(ids).to(dev), B, 3, "linf", SEED, torch.from_numpy(ist).to(dev))
    g = v.cpu().numpy()
    want = H.ref_hsj_estimate(phi, ids, 3, per, "linf", SEED)
    assert (g[1] == 9.0).all() and np.array_equal(_bits(g[[0, 2]]), _bits(want[[0, 2]]))       # a sample that is not live is skipped
    with pytest.raises(ValueError, match="1 .. 4096 probes"):
        K.hsj_estimate(v, torch.zeros(B + 1, N, dtype=torch.int8, device=dev), torch.from_numpy(ids).to(dev), B + 1, 0, "linf", SEED)
    with pytest.raises(ValueError, match="phi must be"):         # fewer rows than probes
        K.hsj_estimate(v, torch.zeros(5, N, dtype=torch.int8, device=dev), torch.from_numpy(ids).to(dev), 6, 0, "linf", SEED)


# ---- 4. ud_hsj_control ----------------------------------------------------------------------------------------------------------------
VALUES = torch.tensor([float("-inf"), -1.0, 0.0, 0.0, 0.5, 0.5, 2.0, float("inf")])
SEQUENCE = ["clean", "start", "start_noise", "start_noise", "begin", "bisect", "bisect", "bisect", "dist", "probe", "probe", "probe",
            "vnorm", "step", "step", "begin", "bisect", "dist", "probe", "vnorm", "step", "begin", "bisect", "dist", "probe", "dist"]


@pytest.mark.parametrize("norm", H.NORMS)
@pytest.mark.parametrize("C", [1, 2, 5])
@pytest.mark.parametrize("N", [1, 5, 300])
def test_control_every_mode_exact_vs_restatement(N, C, norm):
    """A schedule's worth of modes (and three DIST steps: past `steps` nothing is written) over random logits with ties,
    infinities and NaN rows: every table equals the Python restatement's after every launch."""
    from unidefense_amd import kernels as K
    dev = _dev()
    steps, max_probes = 2, 2                                     # the third probe of an iteration and the third DIST find no row
    Q = sum(m in K._HSJ_JUDGES for m in SEQUENCE) - 2            # the last two judged queries find no row of decisions either
    gen = torch.Generator().manual_seed(N * 7 + C)
    ist, fst, nrm, phi, dec, hist = K.hsj_state(N, Q, steps, max_probes, dev)
    dec.fill_(-7)
    phi.fill_(-7)
    hist.fill_(-7.0)
    k = H.hsj_constants(3072, norm, steps, (LO, HI))
    xis = torch.from_numpy(k["xis"]).to(dev)
    y = torch.randint(0, max(C, 2), (N,), generator=gen)
    r = {"ist": ist.cpu().numpy(), "fst": fst.cpu().numpy(), "phi": phi.cpu().numpy(), "dec": dec.cpu().numpy(), "hist": hist.cpu().numpy()}
    consts = dict(delta0=float(k["delta0"]), inv_d=float(k["inv_d"]), dfloor=float(k["dfloor"]))
    for i, mode in enumerate(SEQUENCE):
        logits = VALUES[torch.randint(0, len(VALUES), (N, C), generator=gen)]
        if N > 1 and i < 2:                                      # rows 0 and 2 are not misclassified, row 1 is; row 0 finds its start
            for n, adversarial in ((0, i == 1), (1, True), (2, False)):
                cls = (int(y[n]) + int(adversarial)) % max(C, 2)
                logits[n] = (2.0 * cls - 1.0) if C == 1 else torch.nn.functional.one_hot(torch.tensor(cls), C).float() * 2.0
        logits[(i + 3) % N] = float("nan") if C == 1 else torch.tensor([float("nan")] + [1.0] * (C - 1))[torch.randperm(C, generator=gen)]
        norms = torch.rand(2, N, generator=gen, dtype=torch.float64) * (1e-3 if i % 5 == 0 else 2.0)
        if i % 7 == 0:
            norms[0, 0] = 0.0
        nrm.copy_(norms)
        K.hsj_control(mode, norm, ist, fst, logits=logits.to(dev), y=y.to(dev), nrm=nrm, phi=phi, decisions=dec, history=hist, xis=xis,
                      **consts)
        HC.ref_hsj_control(mode, norm, r["ist"], r["fst"], K.HSJ_I, K.HSJ_F, logits=logits.numpy(), y=y.numpy(), nrm=norms.numpy(),
                          phi=r["phi"], decisions=r["dec"], history=r["hist"], xis=k["xis"], **consts)
        torch.cuda.synchronize()
        assert np.array_equal(ist.cpu().numpy(), r["ist"]), (i, mode)
        assert np.array_equal(_bits(fst), _bits(r["fst"])), (i, mode)
        assert np.array_equal(phi.cpu().numpy(), r["phi"]) and np.array_equal(dec.cpu().numpy(), r["dec"]), (i, mode)
        assert np.array_equal(_bits(hist), _bits(r["hist"])), (i, mode)
    I = K.HSJ_I
    assert (r["ist"][I["k"]] == Q + 2).all() and (r["ist"][I["t"]] == 4).all()
    if N > 1:
        assert r["ist"][I["flags"]].any() and (r["dec"] == 1).any() and (r["dec"] == 0).any() and (r["dec"] == -1).any()
        assert (r["ist"][I["done0"]] == 1).any() and (r["ist"][I["has"]] == 1).any()


# ---- 5. the runner with a known classifier ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", H.NORMS)
def test_runner_decisions_are_the_restatements_row_for_row(norm):
    """UDR18 at 128 x 128 (the smallest size this suite runs the model at), N = 5.  The classifier is the hook: tests/hsj_case.py's
    linear classifier, built at this size, evaluated as x_try.double() on the device; the model's forward runs and is ignored.
    Eager, capturing and replaying call: `decisions` is the numpy restatement's table row for row; radius, history and queries
    match to 1e-6; x_adv is within one fp32 rounding of the restated expressions.  Then the same batch permuted, with permuted
    ids; and a label flipped (radius 0).  The restatement's smallest |margin| over all counted queries is far above what the
    two float64 dot products can differ by."""
    dev = _dev()
    c = HC.make(norm, HC.GPU_SIZE)
    kw = HC.GPU[norm]
    margins = []
    ref = H.ref_hsj(HC.decider(c, margins), c["x"], c["y"], c["ids"], norm=norm, x_init=c["x_init"], **kw)
    clear = float(np.abs(np.array(margins))[ref["decisions"] >= 0].min())
    print(f"  {norm}: restatement's smallest |margin| {clear:.3e}  queries {ref['queries'].tolist()}  radius {ref['radius'].tolist()}")
    assert clear >= 1e-9 and ref["found"].all()
    assert (H.hsj_probe_counts(kw["steps"], kw["probes"], kw["max_probes"])[-1]) == kw["max_probes"]       # B_t is capped here
    wd = torch.from_numpy(c["w"]).to(dev)
    td = torch.from_numpy(c["t"]).to(dev)

    def logits(out, xt):
        m = (xt.double().reshape(xt.shape[0], -1) * wd).sum(1) - td          # float64: the class is 1 where w . x - t > 0
        return torch.stack([-m.sign(), m.sign()], 1).float()
    r = H.HSJRunner(_shared("UDR18", dev), HC.N, HC.GPU_SIZE, norm=norm, logits=logits, **kw)
    x, y, ids, x_init = (torch.from_numpy(c[k]).to(dev) for k in ("x", "y", "ids", "x_init"))

    def check(got, want, perm=None):
        p = np.arange(HC.N) if perm is None else perm
        assert got is r.radius and got.dtype == torch.float32 and r.decisions.dtype == torch.int8
        assert np.array_equal(r.decisions.cpu().numpy(), want["decisions"][:, p])
        assert np.array_equal(r.queries.cpu().numpy(), want["queries"][p]) and not r.flags.any()
        assert np.array_equal(r.found.cpu().numpy(), want["found"][p])
        rel = float(np.abs(got.cpu().numpy().astype(np.float64) / want["radius"][p] - 1).max())
        hrel = float(np.abs(r.history.cpu().numpy().astype(np.float64) / want["history"][:, p] - 1).max())
        dx = float(np.abs(r.x_adv.cpu().numpy().astype(np.float64) - want["x_adv"][p]).max())
        print(f"    radius rel {rel:.3e}  history rel {hrel:.3e}  max |x_adv - restatement| {dx:.3e}")
        assert within(f"hsj known classifier radius {norm}", rel, 1e-6) and within(f"hsj known classifier history {norm}", hrel, 1e-6)
        assert within(f"hsj known classifier x_adv {norm}", dx, 2.0 ** -23)      # one fp32 rounding at |x| <= 1
        assert bool((r.history[1:] <= r.history[:-1]).all())
    for call in range(3):                                        # eager, capture + replay, replay
        got = r(x, y, ids, x_init)
        assert (r.graphs is None) == (call == 0) and tuple(r.decisions.shape) == (r.queries_of(True), HC.N)
        check(got, ref)
    p = np.array([3, 0, 4, 2, 1])
    pt = torch.from_numpy(p).to(dev)
    td.copy_(torch.from_numpy(c["t"][p]).to(dev))                # the classifier's thresholds travel with their samples
    check(r(x[pt], y[pt], ids[pt], x_init[pt]), ref, p)
    td.copy_(torch.from_numpy(c["t"]).to(dev))
    # a flipped label: that sample is already misclassified
    y2 = c["y"].copy()
    y2[1] = 1 - y2[1]
    ref2 = H.ref_hsj(HC.decider(c), c["x"], y2, c["ids"], norm=norm, x_init=c["x_init"], **kw)
    got = r(x, torch.from_numpy(y2).to(dev), ids, x_init)
    assert float(got[1]) == 0.0 and int(r.queries[1]) == 1 and torch.equal(r.x_adv[1], x[1]) and bool(r.found[1])
    assert np.array_equal(r.decisions.cpu().numpy(), ref2["decisions"]) and np.array_equal(r.queries.cpu().numpy(), ref2["queries"])
    # without x_init: one query fewer, the start comes from the noise trials
    ref3 = H.ref_hsj(HC.decider(c), c["x"], c["y"], c["ids"], norm=norm, **kw)
    r(x, y, ids)
    assert tuple(r.decisions.shape) == (r.queries_of(False), HC.N) and np.array_equal(r.decisions.cpu().numpy(), ref3["decisions"])
    assert np.array_equal(r.found.cpu().numpy(), ref3["found"])
    fin = ref3["found"]
    assert np.array_equal(np.isinf(r.radius.cpu().numpy()), ~fin) and torch.equal(r.x_adv[torch.from_numpy(~fin).to(dev)], x[torch.from_numpy(~fin).to(dev)])


# ---- 6. life cycle and real forwards ------------------------------------------------------------------------------------------------------
CASES = [("UDR18", 128, 2, "fp32"), ("UDEB4", 256, 1, "fp32"), ("UDEB4", 256, 1, "fp16")]
REAL = dict(steps=2, probes=8, max_probes=1000, bisect=4, halvings=3, init_trials=2, seed=SEED)
KEEP = ("radius", "found", "x_adv", "queries", "history", "decisions", "flags")


def _cls_out(r, x):
    from unidefense_amd.infer import _eval_nodes
    with torch.no_grad(), _eval_nodes(r.model, r.half):
        return r.model(x)


def _forward(r, x):
    """the label the runner's own eval forward (and its hook, if any) gives x"""
    out = _cls_out(r, x)
    return (out["cls_out"] if r.logits is None else r.logits(out, x)).float().argmax(1)


def _gap(r, x):
    z = _cls_out(r, x)["cls_out"].float()
    return z[:, 0] - z[:, 1]


@functools.lru_cache(maxsize=None)
def _attacked(name, size, n, precision, norm):
    """the eager first call, then two replays; shared by the tests below and left unchanged.  y is the label of x; x_init is one
    of a handful of other images (other seeds, constant images) with another label.  UDR18: the model's own argmax.  UDEB4 with
    the suite's filled parameters answers class 0 for every image (its two logits move by 0.01 over all inputs: a saturated
    head), so its decision is recalibrated by a hook on the REAL forward's output: class 0 where logit0 - logit1 is above a
    per-sample threshold halfway between its value at x and at the candidate that moves it most."""
    dev = _dev()
    m = _shared(name, dev)
    flags = [(p.requires_grad, p.grad is None) for p in m.parameters()]
    values = [t.detach().clone() for t in list(m.parameters()) + list(m.buffers())]
    x = param_fill.make_input(n, size, 5).to(dev)
    cands = [param_fill.make_input(n, size, s).to(dev) for s in (6, 7, 8)] + [torch.full_like(x, v) for v in (-1.0, 1.0, 0.0)]
    x_init, hook = x.clone(), None
    if name == "UDEB4":
        tau = torch.zeros(n, device=dev)

        def calibrated_gap(out, xt):
            z = out["cls_out"].float()
            return torch.stack([z[:, 0] - z[:, 1] - tau, torch.zeros_like(tau)], 1)
        hook = calibrated_gap
    r = H.HSJRunner(m, n, size, norm=norm, precision=precision, logits=hook, **REAL)
    if name == "UDEB4":
        d0, far, d1 = _gap(r, x), torch.zeros(n, device=dev), _gap(r, x)
        for cand in cands:
            d = _gap(r, cand)
            take = (d - d0).abs() > far
            x_init[take], far, d1 = cand[take], torch.where(take, (d - d0).abs(), far), torch.where(take, d, d1)
        tau.copy_(d0 + 0.5 * (d1 - d0))
        have = far > 0
        y = _forward(r, x)
        assert bool((_forward(r, x_init) != y)[have].all())
    else:
        y = _forward(r, x)
        have = torch.zeros(n, dtype=torch.bool, device=dev)
        for cand in cands:
            take = (_forward(r, cand) != y) & ~have
            x_init[take] = cand[take]
            have |= take
    ids = torch.arange(n, dtype=torch.int64, device=dev) + 40
    snap = lambda: {k: getattr(r, k).clone() for k in KEEP}      # noqa: E731
    r(x, y, ids, x_init)
    assert r.graphs is None and r.calls == 1
    warm = snap()
    runs = []
    for _ in range(2):
        r(x, y, ids, x_init)
        runs.append(snap())
    torch.cuda.synchronize()
    assert r.graphs is not None and len(r.graphs) == 6
    return {"runner": r, "x": x, "y": y, "ids": ids, "x_init": x_init, "have": have, "warm": warm, "runs": runs, "flags": flags,
            "values": values}


@pytest.mark.parametrize("norm", H.NORMS)
@pytest.mark.parametrize("name,size,n,precision", CASES)
def test_runner_life_cycle_and_what_it_leaves(name, size, n, precision, norm):
    a = _attacked(name, size, n, precision, norm)
    r, x, y = a["runner"], a["x"], a["y"]
    assert r.args == {"method": "hsj", "norm": norm, "steps": 2, "probes": 8, "max_probes": 1000, "bisect": 4, "halvings": 3,
                      "init_trials": 2, "seed": SEED, "clip": (-1.0, 1.0), "logits": "calibrated_gap" if name == "UDEB4" else None,
                      "precision": precision}
    for k in KEEP:                                               # two replays are bitwise equal, and equal the eager first call
        assert torch.equal(a["runs"][0][k], a["runs"][1][k]), k
        assert torch.equal(a["runs"][0][k], a["warm"][k]), k
    s = a["runs"][0]
    Q = r.queries_of(True)
    assert Q == 1 + 1 + 2 + 3 * 4 + (8 + 11) + 2 * 3 and tuple(s["decisions"].shape) == (Q, n) and s["decisions"].dtype == torch.int8
    assert s["radius"].dtype == torch.float32 and s["found"].dtype == torch.bool and s["queries"].dtype == torch.int32
    assert tuple(s["history"].shape) == (3, n) and bool((s["history"][1:] <= s["history"][:-1]).all())
    assert bool((s["queries"] <= Q).all()) and bool((s["queries"] >= 1).all()) and not bool(s["flags"].any())
    assert torch.equal((s["decisions"] >= 0).sum(0).to(torch.int32), s["queries"])
    assert bool((s["decisions"][0] == 0).all())                  # y is the model's own label: the clean query is not adversarial
    found = s["found"]
    print(f"  {name} {precision} {norm}: start known {a['have'].tolist()}  found {found.tolist()}  radius {s['radius'].tolist()}  "
          f"queries {s['queries'].tolist()}")
    assert torch.equal(found, torch.isfinite(s["radius"])) and bool((found | ~a["have"]).all())      # a known start is used
    assert bool(a["have"].any())                                 # and the case has one
    assert torch.equal(s["x_adv"][~found], x[~found]) and float(s["x_adv"].min()) >= -1.0 and float(s["x_adv"].max()) <= 1.0
    if bool(found.any()):
        assert bool((_forward(r, s["x_adv"]) != y)[found].all())             # the model's own eval forward: adversarial
        d = (s["x_adv"].double() - x.double()).reshape(n, -1)
        norms = d.norm(dim=1) if norm == "l2" else d.abs().amax(1)
        rel = float(((s["radius"].double() - norms).abs() / norms)[found].max())
        print(f"    max |radius - float64 norm of x_adv - x| / norm {rel:.3e}")
        assert within(f"hsj radius vs float64 norm {name} {precision} {norm}", rel, 1e-5)
        assert bool((s["radius"][found] > 0).all())
    m = r.model
    assert not m.training and [(p.requires_grad, p.grad is None) for p in m.parameters()] == a["flags"]
    assert all(torch.equal(t, v) for t, v in zip(list(m.parameters()) + list(m.buffers()), a["values"]))      # values too
    assert set(r.out) >= {"cls_out"} and tuple(r.out["cls_out"].shape) == (n, 2)


def test_a_second_runner_does_not_disturb_the_first_and_inputs_are_checked():
    dev = _dev()
    a = _attacked("UDR18", 128, 2, "fp32", "l2")
    r, x, y, ids, x_init = (a[k] for k in ("runner", "x", "y", "ids", "x_init"))
    m = r.model
    r2 = m.hsj_runner(2, 128, norm="linf", **dict(REAL, steps=1))
    assert r2 is m.hsj_runner(2, 128, norm="linf", **dict(REAL, steps=1)) and r2 is not r and r2.args["steps"] == 1
    r2(x, y, ids, x_init)
    r2(x, y, ids, x_init)
    r(x, y, ids, x_init)
    for k in KEEP:
        assert torch.equal(getattr(r, k), a["runs"][0][k]), k
    calls = r.calls
    for bad, text in ((lambda: r(x.cpu(), y), "cuda"), (lambda: r(x[:1], y), "differs from the runner's key"),
                      (lambda: r(x, y.int()), "differ from the runner's key"), (lambda: r(x, y, ids.int()), "ids must be an int64 tensor"),
                      (lambda: r(x, y, ids, x_init[:1]), "x_init must be a cuda fp32 tensor"),
                      (lambda: r(x, y, ids, x_init.double()), "x_init must be a cuda fp32 tensor")):
        with pytest.raises(ValueError, match=text):
            bad()
    assert r.calls == calls
    # NaN logits: the query counts as not adversarial and sets the flag
    nan_row = torch.tensor([[float("nan"), 0.0], [0.0, 1.0]], device=dev)
    r3 = H.HSJRunner(m, 2, 128, logits=lambda out, xt: nan_row, **dict(REAL, steps=1))
    for _ in range(3):
        radius = r3(x, torch.zeros(2, dtype=torch.int64, device=dev), ids)
        assert r3.flags.tolist() == [1, 0] and math.isinf(float(radius[0])) and not bool(r3.found[0])      # never adversarial: no start
        assert float(radius[1]) == 0.0 and int(r3.queries[1]) == 1 and int(r3.queries[0]) == 1 + 2          # class 1 != y: misclassified
    with pytest.raises(ValueError, match=r"logits must be a \[2, C\] tensor"):
        H.HSJRunner(m, 2, 128, logits=lambda out, xt: nan_row[0], **REAL)(x, y)


# ---- 7. the stage ---------------------------------------------------------------------------------------------------------------------
def test_engine_test_robust_hsj():
    _dev()
    from tests.test_d_train_engine import CONFIG
    from unidefense_amd.attack import robust_curve
    from unidefense_amd.engine import get_engine
    cfg = copy.deepcopy(CONFIG)
    cfg["model"] = {"name": "UDR18", "num_classes": 2, "drop_rate": 0.2}
    cfg["data"] = {"train_batch_size": 2, "size": 128}
    eng = get_engine("FE")(cfg, "Test")
    param_fill.fill_module_(eng.model_without_ddp, sf_coef=0.0, fuse_coef=0.3)
    attack = {"method": "hsj", "norm": "l2", "steps": 1, "probes": 6, "bisect": 4, "halvings": 2, "init_trials": 2, "seed": 3}
    with pytest.raises(ValueError, match="attack method 'hsj' takes HSJRunner's keyword arguments and 'eps'"):
        eng.test_robust(batches=1, attack=dict(attack, stepz=3))
    res = {eps: eng.test_robust(batches=2, attack=dict(attack, eps=eps)) for eps in (0.0, float("inf"))}
    for eps, r in res.items():
        assert set(r) == {"clean", "adv", "attack"}
        a = r["attack"]
        assert a["method"] == "hsj" and a["norm"] == "l2" and a["eps"] == eps and a["steps"] == 1
        assert tuple(a["radius"].shape) == (8,) == tuple(a["found"].shape) and a["radius"].device.type == "cpu"
        assert a["median_radius"] == float(a["radius"].double().median())
        assert torch.equal(a["found"].bool(), torch.isfinite(a["radius"]))
    labels = res[0.0]["clean"]["labels"]
    wrong = (res[0.0]["clean"]["scores"] < 0.5).long() != labels
    assert torch.equal(res[0.0]["attack"]["radius"], res[math.inf]["attack"]["radius"])          # the same streams: the same attack
    assert bool((res[0.0]["attack"]["radius"][wrong] == 0).all()) and bool((res[0.0]["attack"]["radius"][~wrong] > 0).all())
    assert torch.equal(res[0.0]["adv"]["scores"], res[0.0]["clean"]["scores"]) and res[0.0]["adv"]["acc"] == res[0.0]["clean"]["acc"]
    assert res[math.inf]["adv"]["acc"] <= res[math.inf]["clean"]["acc"]
    assert torch.equal(res[0.0]["clean"]["scores"], eng.test(batches=2)["scores"])
    curve = robust_curve(res[0.0]["attack"]["radius"], torch.tensor([0.0, 1e9]))
    assert float(curve[0]) == float((~wrong).double().mean()) and float(curve[1]) == float(torch.isinf(res[0.0]["attack"]["radius"]).double().mean())
    assert all(p.grad is None for p in eng.model_without_ddp.parameters())
