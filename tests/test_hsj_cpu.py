"""CPU: the decision-based minimum-norm attack's restatement (unidefense_amd/hsj.py: ref_hsj and its pieces) on a linear
classifier with a closed-form answer, its edge cases, the schedule, the argument refusals and the C ABI's new entry points."""
import ctypes
import re

import numpy as np
import pytest
import torch

from tests import hsj_case as HC
from unidefense_amd import hsj as H
from unidefense_amd.smooth import ref_smooth_unit


def _model():
    from unidefense_amd.model import load_model
    return load_model("UDR18")(num_classes=2).eval()


# ---- 1. the linear classifier ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", H.NORMS)
def test_linear_classifier_reaches_the_closed_form(norm):
    """sign(w . x - t_n) in float64, N = 5, D = 3072 (tests/hsj_case.py).  The closed-form distance to the boundary is
    |w . x - t| / |w|_2 (L2) and |w . x - t| / |w|_1 (Linf); the clip box is idle at the projection.  Reached radius / closed form
    with the schedules of hsj_case.CPU (seed 3), per sample:
      l2   (steps 18, probes 200, 11090 queries): 1.2146 1.2088 1.2119 1.2183 1.2112
      linf (steps 12, probes  60,  2122 queries): 1.1634 1.1819 1.1558 1.1882 1.1821
    The L2 figure is set by probes / D alone (the estimate is rotation invariant: its cosine with the normal is about
    0.8 sqrt(B / D) per iteration), which is why it takes three times D probes in all."""
    c = HC.make(norm)
    margins = []
    r = H.ref_hsj(HC.decider(c, margins), c["x"], c["y"], c["ids"], norm=norm, x_init=c["x_init"], **HC.CPU[norm])
    kw = HC.CPU[norm]
    Q = H.hsj_queries(kw["steps"], kw["probes"], kw["max_probes"], kw["bisect"], kw["halvings"], kw["init_trials"], True)
    assert r["decisions"].shape == (Q, HC.N) == (len(margins), HC.N) and r["decisions"].dtype == np.int8
    assert r["found"].all() and not r["flags"].any()
    xa = r["x_adv"]
    assert xa.dtype == np.float32 and float(xa.min()) >= -1.0 and float(xa.max()) <= 1.0
    assert (HC.decider(c)(xa) != c["y"]).all()                   # every x_adv is adversarial
    assert (np.diff(r["history"], axis=0) <= 0).all() and np.array_equal(r["history"][-1], r["radius"])
    d = (xa.astype(np.float64) - c["x"].astype(np.float64)).reshape(HC.N, -1)
    measured = np.sqrt((d * d).sum(1)) if norm == "l2" else np.abs(d).max(1)
    assert np.allclose(r["radius"], measured, rtol=1e-6, atol=0)  # the radius is the measured norm, not the search's alpha
    ratio = r["radius"] / c["closed"]
    print(f"  {norm}: radius / closed form {np.round(ratio, 4).tolist()}  queries {r['queries'].tolist()}")
    assert (r["radius"] >= (1 - 1e-6) * c["closed"]).all()
    assert (ratio <= 1.25).all()
    assert (r["queries"] <= Q).all() and (r["queries"] >= Q - kw["init_trials"] - kw["steps"] * kw["halvings"]).all()
    # the counted queries are the decisions that are not -1
    assert np.array_equal((r["decisions"] >= 0).sum(0), r["queries"])


# ---- 2. edge cases -----------------------------------------------------------------------------------------------------------------
SMALL = dict(steps=2, probes=6, max_probes=8, bisect=8, halvings=3, init_trials=3, seed=5)


def test_already_misclassified_no_start_and_invalid_rows():
    c = HC.make("linf")
    y = c["y"].copy()
    y[1] = 1 - y[1]                                              # sample 1 is already misclassified
    Q = H.hsj_queries(2, 6, 8, 8, 3, 3, True)
    r = H.ref_hsj(HC.decider(c), c["x"], y, c["ids"], norm="linf", x_init=c["x_init"], **SMALL)
    assert r["radius"][1] == 0.0 and r["found"][1] and r["queries"][1] == 1 and np.array_equal(r["x_adv"][1], c["x"][1])
    assert r["decisions"][0, 1] == 1 and (r["decisions"][1:, 1] == -1).all() and (r["history"][:, 1] == 0).all()
    assert r["decisions"].shape[0] == Q
    # a classifier that never changes its mind: no start, inf, x_adv = x, queries = clean + x_init + the noise trials
    r = H.ref_hsj(lambda xt: c["y"], c["x"], c["y"], c["ids"], norm="l2", x_init=c["x_init"], **SMALL)
    assert np.isinf(r["radius"]).all() and not r["found"].any() and np.array_equal(r["x_adv"], c["x"])
    assert r["queries"].tolist() == [1 + 1 + 3] * HC.N and np.isinf(r["history"]).all()
    assert (r["decisions"][:5] == 0).all() and (r["decisions"][5:] == -1).all()
    # without x_init the schedule is one query shorter
    r = H.ref_hsj(lambda xt: c["y"], c["x"], c["y"], c["ids"], norm="l2", **SMALL)
    assert r["decisions"].shape[0] == Q - 1 and r["queries"].tolist() == [1 + 3] * HC.N
    # an invalid row (-1) counts as not adversarial and sets bit 0 of flags, for the samples that took part
    calls = []

    def decide(xt):
        calls.append(1)
        cls = HC.decider(c)(xt)
        if len(calls) == 4:
            cls = cls.copy()
            cls[:] = -1
        return cls
    r = H.ref_hsj(decide, c["x"], y, c["ids"], norm="linf", x_init=c["x_init"], **SMALL)
    part = r["decisions"][3] >= 0
    assert part.any() and not part[1] and np.array_equal(r["flags"], part.astype(np.int32)) and (r["decisions"][3][part] == 0).all()


def test_all_equal_phi_and_the_weights():
    ids, per = np.array([5, 9], dtype=np.int64), 10
    u = [ref_smooth_unit(ids, 7 + b, per, "uniform", 11) for b in range(3)]
    total = (u[0] + u[1]) + u[2]
    ones, zeros = np.ones((3, 2), dtype=np.int8), np.zeros((3, 2), dtype=np.int8)
    assert np.array_equal(H.ref_hsj_estimate(ones, ids, 7, per, "linf", 11), np.sign(total))
    assert np.array_equal(H.ref_hsj_estimate(zeros, ids, 7, per, "linf", 11), -np.sign(total))
    z = [ref_smooth_unit(ids, 7 + b, per, "gaussian", 11) for b in range(3)]
    assert np.allclose(H.ref_hsj_estimate(ones, ids, 7, per, "l2", 11, exact=True), z[0] + z[1] + z[2], rtol=0, atol=1e-15)
    assert np.allclose(H.ref_hsj_estimate(zeros, ids, 7, per, "l2", 11, exact=True), -(z[0] + z[1] + z[2]), rtol=0, atol=1e-15)
    mixed = np.array([[1, 0], [0, 0], [0, 1]], dtype=np.int8)
    w = H._weights(mixed)
    third = np.float32(1.0) * (np.float32(1.0) / np.float32(3.0))
    assert w.dtype == np.float32 and np.array_equal(w[:, 0], np.array([1, 0, 0], np.float32) - third)
    want = (w[0][:, None] * z[0] + w[1][:, None] * z[1]) + w[2][:, None] * z[2]
    assert np.allclose(H.ref_hsj_estimate(mixed, ids, 7, per, "l2", 11, exact=True), want, rtol=0, atol=1e-15)
    got32 = H.ref_hsj_estimate(mixed, ids, 7, per, "l2", 11)
    assert got32.dtype == np.float32 and np.abs(got32 - want).max() <= 3 * 2.0 ** -23 * np.abs(want).max() + 1e-7


def test_schedule_counts_and_constants():
    assert H.hsj_probe_counts(5, 100, 150) == [100, 141, 150, 150, 150]          # floor(100 sqrt(2)) = 141, then the cap
    assert H.hsj_probe_counts(3, 1, 1000) == [1, 1, 1] and H.hsj_probe_counts(4, 7, 1000) == [7, 9, 12, 14]
    assert H.hsj_queries(5, 100, 150, 12, 10, 16) == 1 + 16 + 6 * 12 + 691 + 50
    assert H.hsj_queries(5, 100, 150, 12, 10, 16, True) == H.hsj_queries(5, 100, 150, 12, 10, 16) + 1
    k = H.hsj_constants(3072, "l2", 3, (-1, 1))
    assert k["delta0"] == np.float32(0.2) and k["inv_d"] == np.float32(1 / 3072) and k["aux"] == np.float32(1 / np.sqrt(3072))
    assert k["dfloor"] == np.float32(2.0 ** -19 * np.sqrt(3072)) and H.hsj_constants(3072, "linf", 3, (-1, 1))["dfloor"] == 2.0 ** -19
    assert k["xis"].dtype == np.float32 and np.array_equal(k["xis"], (1 / np.sqrt([1.0, 2.0, 3.0])).astype(np.float32))


def test_a_permuted_batch_with_permuted_ids_gives_permuted_results():
    """The attack on a sample is a function of (seed, id, the model's decisions): not of its row, not of N."""
    c = HC.make("linf")
    kw = dict(SMALL, steps=3, probes=10, max_probes=20, bisect=12)
    a = H.ref_hsj(HC.decider(c), c["x"], c["y"], c["ids"], norm="linf", x_init=c["x_init"], **kw)
    p = np.array([3, 0, 4, 2, 1])
    cp = dict(c, t=c["t"][p])
    b = H.ref_hsj(HC.decider(cp), c["x"][p], c["y"][p], c["ids"][p], norm="linf", x_init=c["x_init"][p], **kw)
    for name in ("radius", "found", "x_adv", "queries", "flags"):
        assert np.array_equal(b[name], a[name][p]), name
    assert np.array_equal(b["history"], a["history"][:, p]) and np.array_equal(b["decisions"], a["decisions"][:, p])
    # one sample alone
    one = dict(c, t=c["t"][2:3])

    def decide1(xt):
        return (np.asarray(xt).reshape(1, -1).astype(np.float64) @ c["w"] - one["t"] > 0).astype(np.int64)
    s = H.ref_hsj(decide1, c["x"][2:3], c["y"][2:3], c["ids"][2:3], norm="linf", x_init=c["x_init"][2:3], **kw)
    assert s["radius"][0] == a["radius"][2] and np.array_equal(s["x_adv"][0], a["x_adv"][2])
    assert np.array_equal(s["decisions"][:, 0], a["decisions"][:, 2])


def test_propose_restatement_forms():
    a = np.array([[0.5, -0.25, 0.9]], dtype=np.float32)
    b = np.array([[0.0, 0.25, 0.95]], dtype=np.float32)
    s = np.array([0.25], dtype=np.float32)
    assert H.ref_hsj_propose("bisect", "l2", a, b, s, None, -1, 1).tolist() == [[0.125, 0.125, np.float32(0.95) + np.float32(0.25) * (a[0, 2] - b[0, 2])]]
    assert H.ref_hsj_propose("bisect", "linf", a, b, s, None, -1, 1).tolist() == [[0.25, 0.0, a[0, 2]]]
    assert np.array_equal(H.ref_hsj_propose("settle", "l2", a, b, np.array([1.0], np.float32), None, -1, 1, plain=np.array([True])), a)
    t = np.array([[1.0, -1.0, 0.5]], dtype=np.float32)
    assert H.ref_hsj_propose("noise", "linf", None, None, None, t, -1, 0.5).tolist() == [[0.5, -1.0, 0.125]]
    assert H.ref_hsj_propose("probe", "linf", a, None, s, t, -1, 1).tolist() == [[0.75, -0.5, 1.0]]
    assert H.ref_hsj_propose("step", "l2", a, t, s, None, -1, 1).tolist() == [[0.75, -0.5, 1.0]]
    assert H.ref_hsj_propose("probe", "l2", a, None, s, t.astype(np.float64), -1, 1).dtype == np.float64


# ---- 3. refusals, the accessor, the keys -------------------------------------------------------------------------------------------------
BAD = [({"norm": "l1"}, "norm must be one of ('l2', 'linf')"), ({"norm": None}, "norm must be one of"),
       ({"targeted": True}, "untargeted"), ({"steps": 0}, "steps must be an integer >= 1"), ({"steps": 2.5}, "steps must be an integer >= 1"),
       ({"probes": 0}, "probes must be an integer >= 1"), ({"max_probes": 0}, "max_probes must be an integer >= 1"),
       ({"max_probes": 4097}, "max_probes must be at most 4096"), ({"bisect": 0}, "bisect must be an integer >= 1"),
       ({"halvings": 0}, "halvings must be an integer >= 1"), ({"init_trials": -1}, "init_trials must be an integer >= 0"),
       ({"init_trials": True}, "init_trials must be an integer >= 0"), ({"seed": 1.5}, "seed must be an integer"),
       ({"clip": (1.0, -1.0)}, "clip must be (lo, hi) with lo < hi"), ({"clip": (0.0, float("inf"))}, "clip must be finite"),
       ({"clip": (0.0,)}, "clip must be"), ({"logits": "cls_out"}, "logits must be None or a callable"),
       ({"steps": 600000, "probes": 1 << 12, "max_probes": 4096}, "must stay below 2^31"),
       ({"precision": "bf16"}, "precision"), ({"precision": "fp16"}, "fp16")]


@pytest.mark.parametrize("kw,text", BAD)
def test_refusals_need_no_device(kw, text):
    m = _model()
    for make in (lambda: H.HSJRunner(m, 2, 64, **kw), lambda: H.hsj_runner(m, 2, 64, **kw), lambda: m.hsj_runner(2, 64, **kw)):
        with pytest.raises(ValueError, match=re.escape(text)):
            make()
    assert not m.__dict__.get("_ud_hsj_runners")


def test_host_side_refusals_defaults_and_keys():
    from unidefense_amd.model import load_model
    m = load_model("UDR18")(num_classes=2)
    with pytest.raises(ValueError, match="eval"):
        H.HSJRunner(m.train(), 2, 64)
    with pytest.raises(ValueError, match="cuda"):                # every argument passed: only the device is missing
        H.HSJRunner(m.eval(), 2, 64, norm="linf", steps=3, probes=5, max_probes=9, bisect=4, halvings=2, init_trials=0, seed=1 << 40,
                    clip=(0.0, 1.0), logits=lambda out, x: x)
    with pytest.raises(ValueError, match="takes a UDEB4"):
        H.HSJRunner(torch.nn.Linear(2, 2), 2, 64)
    for name in ("UDEB4", "UDR18", "UDR50"):
        assert callable(getattr(load_model(name), "hsj_runner"))
    a = H._hsj_arguments(4, 128)
    assert list(a) == ["batch", "size", "norm", "steps", "probes", "max_probes", "bisect", "halvings", "init_trials", "seed", "clip",
                       "precision", "logits", "targeted"]
    assert tuple(a.values())[2:] == ("l2", 20, 100, 1000, 12, 10, 16, 0, (-1.0, 1.0), "fp32", None, False)
    assert H.HSJRunner._backward is False
    assert H.hsj_key(4, 128) == H.hsj_key(4, 128, norm="l2", clip=[-1, 1]) != H.hsj_key(4, 128, norm="linf")
    assert H.hsj_key(4, 128, precision="fp16")[-1] == "fp16" and H.hsj_key(4, 128) == H.hsj_key(4, 128, precision="fp16")[:-1]
    f = lambda out, x: x                                         # noqa: E731
    assert H.hsj_key(4, 128, logits=f) == H.hsj_key(4, 128, logits=f) != H.hsj_key(4, 128)


def test_engine_method_table_and_stage_refusals():
    """"hsj" is test_robust's decision-based method, in a table of its own beside ROBUST; its refusals fire before any batch"""
    from unidefense_amd.engine import evaluate

    class Net:
        def hsj_runner(self, batch, size, **kw):
            raise AssertionError("no runner may be asked for")

    def iterator(step, batch, size, device):
        raise AssertionError("no batch may be drawn")
    assert list(evaluate.ROBUST_DECISION) == ["hsj"] and "hsj" not in evaluate.ROBUST
    ev = evaluate.Evaluator(None, Net(), iterator, 2, 32, "cpu")
    with pytest.raises(ValueError, match="eps must be >= 0"):
        ev.test_robust(1, {"method": "hsj", "eps": -1.0})
    with pytest.raises(ValueError, match="attack method must be"):
        ev.test_robust(1, {"method": "hopskip"})
    with pytest.raises(ValueError, match="attack method 'hsj' takes HSJRunner's keyword arguments and 'eps': .*stepz"):
        ev.test_robust(1, {"method": "hsj", "stepz": 3})         # an unknown key: before any batch, like a bad value


def test_engine_picks_the_next_batch_mate_and_keys_the_streams():
    from unidefense_amd.engine import evaluate
    seen = {}

    class Runner:
        args = {"method": "hsj", "norm": "l2"}

        def __call__(self, x, y, ids, x_init):
            seen.setdefault("ids", []).append(ids.clone())
            seen.setdefault("x_init", []).append(x_init.clone())
            self.x_adv = x + 1.0
            self.found = torch.tensor([True, True, False, True])
            self.radius = torch.tensor([0.0, 0.5, float("inf"), 2.0])
            return self.radius

    class Net:
        def hsj_runner(self, batch, size, **kw):
            seen["kw"] = kw
            return Runner()

    def iterator(step, batch, size, device):
        base = torch.arange(4, dtype=torch.float32).reshape(4, 1, 1, 1).expand(4, 3, 2, 2) + 10 * step
        return base[:2].clone(), torch.zeros(2, dtype=torch.int64), base[2:].clone(), torch.ones(2, dtype=torch.int64)

    class Ev(evaluate.Evaluator):
        def score(self, x):                                      # p(real): samples 0 and 3 are called real (label 0), 1 and 2 fake
            marks = x[:, 0, 0, 0] % 10
            return torch.where((marks == 0) | (marks == 3) | (marks > 3), torch.tensor(0.9), torch.tensor(0.1))

    ev = Ev(None, Net(), iterator, 2, 2, "cpu")
    res = ev.test_robust(2, {"method": "hsj", "norm": "l2", "eps": 1.0, "steps": 3})
    assert seen["kw"] == {"norm": "l2", "steps": 3}
    assert [i.tolist() for i in seen["ids"]] == [[0, 1, 2, 3], [4, 5, 6, 7]]
    # labels (0, 0, 1, 1), clean predictions (0, 1, 1, 0): sample 0 -> mate 1, 1 -> 2, 2 -> 3, 3 -> 0
    assert seen["x_init"][0][:, 0, 0, 0].tolist() == [11.0, 12.0, 13.0, 10.0]
    a = res["attack"]
    assert a["method"] == "hsj" and a["eps"] == 1.0 and a["radius"].tolist() == [0.0, 0.5, float("inf"), 2.0] * 2
    assert a["found"].tolist() == [1, 1, 0, 1] * 2 and a["median_radius"] == 0.5
    assert set(res) == {"clean", "adv", "attack"}


# ---- 4. the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_refuse_bad_arguments():
    from tests.test_abi_cpu import header
    from unidefense_amd import kernels as K
    from unidefense_amd import lib
    h = header()
    L = ctypes.CDLL(lib.LIB_PATH)
    names = ("ud_hsj_propose", "ud_hsj_control", "ud_hsj_dist", "ud_hsj_estimate")
    for n in names:
        assert n in h.protos and n in lib.EXPORTED and hasattr(L, n), n
        fn = getattr(L, n)
        fn.restype, fn.argtypes = ctypes.c_int, [t for t, _ in h.protos[n][1]]
    assert [name for _, name in h.protos["ud_hsj_estimate"][1]] == ["v", "phi", "ids", "ist", "N", "per", "B", "draw0", "norm", "inv_b",
                                                                    "seed", "stream"]
    assert K.HSJ_I == {"active": 0, "has": 1, "moved": 2, "stepdone": 3, "accept": 4, "keep": 5, "k": 6, "draw": 7, "pb": 8, "t": 9,
                       "queries": 10, "flags": 11, "done0": 12}
    assert K.HSJ_F == {"lo": 0, "hi": 1, "delta": 2, "xi": 3, "invn": 4, "dist": 5, "best": 6, "radius": 7}
    assert list(K.HSJ_P) == ["copy", "copy_seek", "noise", "bisect", "settle", "probe", "step"]
    assert list(K.HSJ_C) == ["clean", "start", "start_noise", "bisect", "probe", "step", "begin", "dist", "vnorm"]
    assert K.HSJ_NORM == {"linf": 0, "l2": 1} and K.HSJ_MAX_PROBES == 4096 and set(K.HSJ_NORM) == set(H.NORMS)
    buf = (ctypes.c_double * 96)()
    a, b, c, d, e, f = (ctypes.cast(ctypes.addressof(buf) + 64 * j, ctypes.c_void_p) for j in range(6))
    nan = float("nan")
    # ud_hsj_estimate(v, phi, ids, ist, N, per, B, draw0, norm, inv_b, seed, stream)
    ok = (a, b, c, None, 2, 12, 3, 0, 0, 0.25, 1, None)
    bad = [ok[:i] + (None,) + ok[i + 1:] for i in range(3)]
    bad += [ok[:4] + t + ok[9:] for t in ((0, 12, 3, 0, 0), (65536, 12, 3, 0, 0), (2, 0, 3, 0, 0), (2, 12, 0, 0, 0), (2, 12, 4097, 0, 0),
                                          (2, 12, 3, -1, 0), (2, 12, 3, (1 << 31) - 2, 0), (2, 12, 3, 0, 2), (2, 12, 3, 0, -1))]
    for args in bad:
        assert L.ud_hsj_estimate(*args) == -1000, args
    # ud_hsj_dist(a, b, ist, N, per, out, stream)
    for args in ((None, b, None, 2, 12, c, None), (a, b, None, 2, 12, None, None), (a, b, None, 0, 12, c, None), (a, b, None, 2, 0, c, None)):
        assert L.ud_hsj_dist(*args) == -1000, args
    # ud_hsj_propose(mode, norm, dst, a, b, ids, ist, fst, N, per, lo, hi, aux, seed, stream)
    ok = (3, 1, a, b, c, d, e, f, 2, 12, -1.0, 1.0, 0.5, 1, None)
    bad = [ok[:i] + (None,) + ok[i + 1:] for i in (2, 3, 4, 6, 7)]
    bad += [(7,) + ok[1:], (-1,) + ok[1:], ok[:1] + (2,) + ok[2:], ok[:3] + (a,) + ok[4:], ok[:4] + (a,) + ok[5:],
            ok[:8] + (0,) + ok[9:], ok[:9] + (0,) + ok[10:], ok[:10] + (1.0, 1.0) + ok[12:], ok[:10] + (nan, 1.0) + ok[12:],
            (5,) + ok[1:5] + (None,) + ok[6:]]                   # a noisy mode without ids
    for args in bad:
        assert L.ud_hsj_propose(*args) == -1000, args
    # ud_hsj_control(mode, norm, logits, C, y, nrm, ist, fst, phi, decisions, history, xis, N, Q, max_probes, steps, delta0, inv_d, dfloor, stream)
    ok = (4, 0, a, 2, b, c, d, e, f, a, b, c, 2, 8, 8, 3, 0.2, 0.01, 0.001, None)
    bad = [ok[:i] + (None,) + ok[i + 1:] for i in (2, 4, 6, 7, 8, 9)]
    bad += [(9,) + ok[1:], (-1,) + ok[1:], ok[:1] + (2,) + ok[2:], ok[:3] + (0,) + ok[4:], ok[:12] + (0,) + ok[13:],
            ok[:13] + (0,) + ok[14:], ok[:14] + (4097,) + ok[15:], ok[:14] + (0,) + ok[15:]]
    dist = (7,) + ok[1:]
    bad += [dist[:5] + (None,) + dist[6:], dist[:10] + (None,) + dist[11:], dist[:11] + (None,) + dist[12:], dist[:15] + (0,) + dist[16:],
            dist[:16] + (0.0,) + dist[17:], dist[:17] + (nan,) + dist[18:], dist[:18] + (-1.0,) + dist[19:]]
    for args in bad:
        assert L.ud_hsj_control(*args) == -1000, args


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from unidefense_amd import kernels as K
    x = torch.zeros(2, 3, 4, 4)
    ids = torch.zeros(2, dtype=torch.int64)
    ist, fst = torch.zeros(13, 2, dtype=torch.int32), torch.zeros(8, 2)
    phi = torch.zeros(4, 2, dtype=torch.int8)
    for call in (lambda: K.hsj_propose("probe", "l2", x, x.clone(), None, ids, ist, fst, -1, 1),
                 lambda: K.hsj_dist(x, x.clone(), torch.zeros(2, 2, dtype=torch.float64)),
                 lambda: K.hsj_estimate(x, phi, ids, 3, 0, "l2", 0),
                 lambda: K.hsj_control("clean", "l2", ist, fst, logits=torch.zeros(2, 2), y=ids, decisions=phi)):
        with pytest.raises(ValueError, match="CUDA"):
            call()
