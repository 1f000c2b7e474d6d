"""CPU: the universal perturbation's host side (unidefense_amd/universal.py, engine/evaluate.py: test_universal): every refusal
without a device, the step's resolution, the four entry points' argument tests, the header's rows, the float64 restatements'
properties, the runner cache's key and the stage's rules against stubs."""
import ctypes
import math
import re

import pytest
import torch

from unidefense_amd import universal as U
from unidefense_amd.engine import evaluate, metrics

EPS = 4.0 / 255.0


def _model():
    from unidefense_amd.model import load_model
    return load_model("UDR18")(num_classes=2).eval()


# ---- refusals and resolution -------------------------------------------------------------------------------------------------------
BAD = [({"norm": "l1"}, "norm must be one of ('linf', 'l2')"), ({}, "eps must be >= 0, got None"), ({"eps": -0.1}, "eps must be >= 0"),
       ({"eps": float("nan")}, "eps must be >= 0"), ({"eps": EPS, "steps": 0}, "steps must be an integer >= 1"),
       ({"eps": EPS, "steps": 1.5}, "steps must be an integer >= 1"), ({"eps": EPS, "clip": (1.0, -1.0)}, "clip must be (lo, hi)"),
       ({"eps": EPS, "clip": (0.0,)}, "clip must be (lo, hi)"), ({"eps": EPS, "beta": 0.0}, "beta must be > 0"),
       ({"eps": EPS, "beta": -1.0}, "beta must be > 0"), ({"eps": EPS, "beta": float("nan")}, "beta must be > 0"),
       ({"eps": EPS, "beta": None}, "beta must be > 0"), ({"eps": EPS, "source": 2}, "source must be one of (None, 0, 1)"),
       ({"eps": EPS, "source": -1}, "source must be one of"), ({"eps": EPS, "source": "fake"}, "source must be one of"),
       ({"eps": EPS, "source": 0.5}, "source must be one of"), ({"eps": EPS, "reduce": "sum"}, "reduce must be None or a callable"),
       ({"eps": EPS, "precision": "bf16"}, "precision"), ({"eps": EPS, "precision": "fp16"}, "fp16"),
       ({"eps": EPS, "grad_scale": 3.0}, "grad_scale")]


@pytest.mark.parametrize("kw,text", BAD)
def test_refusals_need_no_device(kw, text):
    m = _model()
    for make in (lambda: U.UniversalRunner(m, 2, 64, **kw), lambda: U.universal_runner(m, 2, 64, **kw),
                 lambda: m.universal_runner(2, 64, **kw)):
        with pytest.raises(ValueError, match=re.escape(text)):
            make()
    assert not m.__dict__.get("_ud_universal_runners")


def test_host_side_refusals_and_pinned_tables():
    from unidefense_amd import attack, corrupt
    from unidefense_amd.model import load_model
    m = load_model("UDR18")(num_classes=2)
    with pytest.raises(ValueError, match="eval"):
        U.UniversalRunner(m.train(), 2, 64, eps=EPS)
    with pytest.raises(ValueError, match="cuda"):            # every argument passed: only the device is missing
        U.UniversalRunner(m.eval(), 2, 64, eps=EPS, norm="l2", beta=1.0, source=1, reduce=lambda g: None)
    with pytest.raises(ValueError, match="takes a UDEB4"):
        U.UniversalRunner(torch.nn.Linear(2, 2), 2, 64, eps=EPS)
    assert attack.NORMS == ("linf", "l2") and U.SOURCES == (None, 0, 1) and len(corrupt.CORRUPTIONS) == 7
    for name in ("UDEB4", "UDR18", "UDR50"):
        assert callable(getattr(load_model(name), "universal_runner"))


def test_step_resolution():
    assert U.resolve_uap_step(EPS) == EPS / 10.0 and U.resolve_uap_step(EPS, None) == EPS / 10.0
    assert U.resolve_uap_step(EPS, 0.25) == 0.25 and U.resolve_uap_step(0.0) == 0.0 and U.resolve_uap_step(EPS, 0) == 0.0
    a = U._universal_arguments(4, 128, eps=EPS)
    assert list(a) == ["batch", "size", "norm", "eps", "steps", "step", "beta", "source", "clip", "precision", "grad_scale", "reduce"]
    assert (a["norm"], a["steps"], a["step"], a["beta"], a["source"], a["clip"], a["precision"], a["reduce"]) == \
        ("linf", 1, None, math.inf, None, (-1.0, 1.0), "fp32", None)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_refuse_bad_arguments():
    from tests.test_abi_cpu import header
    from unidefense_amd import kernels as K
    from unidefense_amd import lib
    h = header()
    L = ctypes.CDLL(lib.LIB_PATH)
    names = ("ud_uap_control", "ud_uap_reduce", "ud_uap_update_linf", "ud_uap_apply")
    for n in names:
        assert n in h.protos and n in lib.EXPORTED and hasattr(L, n), n
        assert h.protos[n][0] is ctypes.c_int, n
        fn = getattr(L, n)
        fn.restype, fn.argtypes = ctypes.c_int, [t for t, _ in h.protos[n][1]]
    assert not any(n.startswith("ud_uap") and n.endswith("_ws_bytes") for n in h.protos)
    for n in ("uap_state", "uap_control", "uap_reduce", "uap_update_linf", "uap_apply"):
        assert callable(getattr(K, n)), n
    # the rows of ist: the header's, and the table kernels.py derives from it
    rows = {k[len("UD_UAP_I_"):].lower(): v for k, v in h.consts.items() if k.startswith("UD_UAP_I_")}
    assert K.UAP_I == rows == {"k": 0}
    buf = (ctypes.c_double * 64)()
    a, b, c, d, e, f = (ctypes.cast(ctypes.addressof(buf) + 64 * j, ctypes.c_void_p) for j in range(6))
    inf, nan = float("inf"), float("nan")
    ok = (a, b, c, d, e, f, 4, 2, inf, -1, None)                      # (f, y, w, ist, history, counted, N, steps, beta, source)
    bad = [ok[:i] + (None,) + ok[i + 1:] for i in range(6)]
    bad += [ok[:6] + t + (None,) for t in ((0, 2, inf, -1), (-1, 2, inf, -1), (4, 0, inf, -1), (4, -3, inf, 0), (4, 2, nan, 1),
                                           (65536, 65536, inf, -1))]
    for args in bad:
        assert L.ud_uap_control(*args) == -1000, args
    ok = (a, b, c, 4, 12, None)                                       # (g, w, gsum, N, per)
    bad = [ok[:i] + (None,) + ok[i + 1:] for i in range(3)] + [(a, b, c, 0, 12, None), (a, b, c, 65536, 12, None), (a, b, c, 4, 0, None),
                                                               (a, b, c, 4, -4, None), (a, b, c, 4, 1 << 39, None)]
    for args in bad:
        assert L.ud_uap_reduce(*args) == -1000, args
    ok = (a, b, c, d, 4, 12, 0.1, 0.1, -1.0, 1.0, None)               # (delta, gsum, x, x_adv, N, per, step, eps, lo, hi)
    bad = [ok[:i] + (None,) + ok[i + 1:] for i in range(4)]
    bad += [ok[:4] + t + (None,) for t in ((0, 12, 0.1, 0.1, -1.0, 1.0), (4, 0, 0.1, 0.1, -1.0, 1.0), (4, 12, nan, 0.1, -1.0, 1.0),
                                           (4, 12, 0.1, -0.1, -1.0, 1.0), (4, 12, 0.1, nan, -1.0, 1.0), (4, 12, 0.1, 0.1, 1.0, -1.0),
                                           (4, 12, 0.1, 0.1, nan, 1.0))]
    for args in bad:
        assert L.ud_uap_update_linf(*args) == -1000, args
    ok = (a, None, c, d, 4, 12, 0.1, -1.0, 1.0, None)                 # (delta, dss, x, x_adv, N, per, eps, lo, hi): dss may be NULL
    bad = [ok[:i] + (None,) + ok[i + 1:] for i in (0, 2, 3)]
    bad += [ok[:4] + t + (None,) for t in ((0, 12, 0.1, -1.0, 1.0), (4, 0, 0.1, -1.0, 1.0), (4, 12, -0.1, -1.0, 1.0),
                                           (4, 12, nan, -1.0, 1.0), (4, 12, 0.1, 1.0, -1.0), (4, 12, 0.1, -1.0, nan))]
    bad += [args[:1] + (b,) + args[2:] for args in bad]               # the same with a dss
    for args in bad:
        assert L.ud_uap_apply(*args) == -1000, args


def test_wrappers_refuse_cpu_tensors():
    from unidefense_amd import kernels as K
    x, d = torch.zeros(2, 3, 4, 4), torch.zeros(3, 4, 4)
    w = torch.zeros(2, dtype=torch.int32)
    for call in (lambda: K.uap_reduce(x, w, d), lambda: K.uap_update_linf(d, d.clone(), x, x.clone(), 0.1, 0.1, -1, 1),
                 lambda: K.uap_apply(d, None, x, x.clone(), 0.1, -1, 1),
                 lambda: K.uap_control(torch.zeros(2), torch.zeros(2, dtype=torch.int64), w, w.view(1, 2), torch.zeros(1, 2),
                                       w.view(1, 2), math.inf)):
        with pytest.raises(ValueError, match="CUDA"):
            call()


# ---- the float64 restatements -----------------------------------------------------------------------------------------------------------
def _case(seed, n=5, per=75):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, per, generator=g), (torch.rand(per, generator=g) * 2 - 1) * EPS, torch.rand(n, per, generator=g) * 2 - 1)


def ref_list(w):
    return [int(v) for v in w]


def test_ref_control_rule():
    f = torch.tensor([0.5, 2.0, float("nan"), 1.0, 0.1])
    y = torch.tensor([0, 1, 1, 0, 1])
    assert ref_list(U.ref_uap_control(f, y)) == [1, 1, 0, 1, 1]                       # beta = inf, source None: everyone (but a NaN)
    assert ref_list(U.ref_uap_control(f, y, beta=1.0)) == [1, 0, 0, 0, 1]             # strict: f == beta is out
    assert ref_list(U.ref_uap_control(f, y, source=1)) == [0, 1, 0, 0, 1]
    assert ref_list(U.ref_uap_control(f, y, beta=1.0, source=0)) == [1, 0, 0, 0, 0]
    assert bool(U.ref_uap_control(torch.rand(64) * 100, torch.zeros(64, dtype=torch.int64)).all())


def test_ref_reduce_skips_the_excluded():
    g, _, _ = _case(1)
    g[1, 3] = float("nan")
    w = torch.tensor([1, 0, 1, 0, 1])
    got = U.ref_uap_reduce(g, w)
    assert got.dtype == torch.float64 and torch.equal(got, g[0].double() + g[2].double() + g[4].double())
    assert torch.isnan(U.ref_uap_reduce(g, torch.ones(5))[3])                         # counted: visible
    assert torch.equal(U.ref_uap_reduce(g, torch.zeros(5)), torch.zeros(75, dtype=torch.float64))


@pytest.mark.parametrize("norm", ["linf", "l2"])
def test_ref_updates_keep_delta_without_weights_and_stay_in_the_budget(norm):
    update = U.ref_uap_update_linf if norm == "linf" else U.ref_uap_update_l2
    g, delta, x = _case(2)
    eps = EPS if norm == "linf" else 0.7 * float(delta.double().norm())
    # nobody counted: gsum is zero, delta stays (L2: 0 / max(0, 1e-12) is 0, not NaN; delta is inside the ball already)
    zero = U.ref_uap_reduce(g, torch.zeros(5))
    inside = delta if norm == "linf" else delta * 0.5
    kept = update(inside, zero, 0.3 * eps, eps)
    assert not torch.isnan(kept).any() and torch.equal(kept, inside.double())
    d = delta.double()
    for seed in range(6):                                  # any update: a large step, a small one, from the last point
        gs = U.ref_uap_reduce(_case(10 + seed)[0], torch.ones(5))
        d = update(d, gs, eps * (3.0 if seed % 2 else 0.1), eps)
        assert float(d.abs().max()) <= eps if norm == "linf" else float(d.norm()) <= eps * (1 + 1e-12)
    wide = x * 1.1                                         # a few values outside the clip
    xa = U.ref_uap_apply(d, wide, -1.0, 1.0)
    assert xa.shape == x.shape and float(xa.min()) >= -1.0 and float(xa.max()) <= 1.0 and float(wide.abs().max()) > 1.0
    assert torch.equal(xa, (wide.double() + d).clamp(-1.0, 1.0))
    assert torch.equal(update(d, gs, 1.0, 0.0), torch.zeros_like(d))                  # eps = 0: the zero pattern


def test_ref_linf_on_hand_values():
    d = torch.tensor([0.0, 0.1, -0.1, 0.05, 0.05])
    gs = torch.tensor([1.0, 2.0, -3.0, 0.0, -0.0])
    got = U.ref_uap_update_linf(d, gs, 0.05, 0.1)
    assert got.dtype == torch.float64
    # a step from 0, two steps cut at +-eps, and sign(0) = sign(-0) = 0: no move
    assert got.tolist() == [0.05, 0.1, -0.1, float(d[3]), float(d[4])]


# ---- the cache's key ----------------------------------------------------------------------------------------------------------------------
def test_cache_key(monkeypatch):
    made = []

    class Stub:
        def __init__(self, model, *args):
            made.append(args)

    monkeypatch.setattr(U, "UniversalRunner", Stub)
    m = _model()

    def hook(gsum):
        return None

    def other(gsum):
        return None

    r = U.universal_runner(m, 4, 128, eps=EPS)
    assert U.universal_runner(m, 4, 128, eps=EPS) is r and m.universal_runner(4, 128, norm="linf", eps=EPS, steps=1) is r
    assert U.universal_runner(m, 4, 128, "linf", EPS, 1, None, math.inf, None) is r and len(made) == 1
    others = [U.universal_runner(m, 4, 128, eps=EPS, **kw) for kw in ({"source": 1}, {"beta": 1.0}, {"reduce": hook})]
    assert len({id(o) for o in others + [r]}) == 4 and len(made) == 4
    assert U.universal_runner(m, 4, 128, eps=EPS, reduce=hook) is others[2]             # a callable is keyed by identity
    assert U.universal_runner(m, 4, 128, eps=EPS, reduce=other) is not others[2]
    # constructor arguments after the model: (batch, size, norm, eps, steps, step, beta, source, ..., reduce)
    assert made[-1][-1] is other and made[3][-1] is hook and made[1][7] == 1 and made[2][6] == 1.0
    from unidefense_amd.infer import _MAX_RUNNERS
    assert len(m.__dict__["_ud_universal_runners"]) <= _MAX_RUNNERS
    assert not any(k.startswith("_ud_") and k != "_ud_universal_runners" for k in m.__dict__)     # a dictionary of its own


# ---- the stage against stubs ----------------------------------------------------------------------------------------------------------------
DEV = torch.device("cpu")


def logits(x):
    return torch.stack([x[:, :1].mean((1, 2, 3)), x[:, 1:].mean((1, 2, 3))], 1) * 8.0


def p0(x):
    return torch.softmax(logits(x), 1)[:, 0]


class Batches:
    """seeded batches of 2 real + 2 fake 3x8x8 images per step; .steps logs the steps drawn"""

    def __init__(self):
        self.steps = []

    def __call__(self, step, batch, size, device):
        self.steps.append(step)
        g = torch.Generator().manual_seed(100 + step)
        xr, xf = (torch.rand(batch, 3, size, size, generator=g) * 2 - 1 for _ in range(2))
        return xr, torch.zeros(batch, dtype=torch.long), xf, torch.ones(batch, dtype=torch.long)

    @staticmethod
    def of(steps, batch=2, size=8):
        parts = [Batches()(s, batch, size, DEV) for s in steps]
        return torch.cat([torch.cat([p[0], p[2]]) for p in parts]), torch.cat([torch.cat([p[1], p[3]]) for p in parts])


class StubRunner:
    """delta's channel 0 grows by 0.1 per call (the fit is visible in the scores); counted: call c counts c % 3 samples"""

    def __init__(self, net, kwargs):
        self.net, self.calls = net, 0
        self.args = dict({"method": "universal", "norm": "linf", "eps": 0.25, "clip": (-1.0, 1.0)}, **kwargs)
        self.delta = torch.zeros(3, 8, 8)
        self.counted = torch.zeros(1, 4, dtype=torch.int32)

    def reset(self):
        self.net.log.append("reset")
        self.delta.zero_()

    def __call__(self, x, y):
        self.net.log.append(("fit", float(x.sum())))
        self.calls += 1
        self.delta[0] += 0.1
        self.counted.zero_()
        self.counted[0, :self.calls % 3] = 1
        return (x + self.delta).clamp(-1, 1)

    def apply(self, x, out=None):
        self.net.log.append("apply")
        return (x + self.delta).clamp(-1, 1)


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.log, self.runner = [], None

    def forward(self, x):
        self.log.append("forward")
        return {"cls_out": logits(x)}

    def universal_runner(self, n, size, norm="linf", eps=0.25, steps=1, reduce=None):
        self.log.append(("universal_runner", n, size))
        if self.runner is None:
            self.runner = StubRunner(self, {"norm": norm, "eps": eps, "steps": steps})
        return self.runner


def make():
    net, it = Net(), Batches()
    return evaluate.Evaluator(net, net, it, 2, 8, DEV), net, it


def expected(scores, labels):
    import numpy as np
    sc, lb = scores.numpy(), labels.numpy()
    ret = {"scores": scores, "labels": labels, "acc": float(np.mean((sc < 0.5).astype(int) == lb))}
    ret.update(metrics.cal_metrics(lb, sc, threshold=0.5))
    return ret


def same(got, want):
    assert set(got) == set(want)
    for k, v in want.items():
        assert torch.equal(got[k], v) if torch.is_tensor(v) else got[k] == v, k


@pytest.mark.parametrize("norm", ["linf", "l2"])
def test_stage_fit_then_held_out_three_ways(norm, monkeypatch):
    gathered = []
    real = metrics.gather_scores
    monkeypatch.setattr(metrics, "gather_scores", lambda s, lb: gathered.append(s) or real(s, lb))
    ev, net, it = make()
    given = {"norm": norm, "eps": 0.25, "seed": 9}
    got = ev.test_universal(2, 3, 2, given)
    assert given == {"norm": norm, "eps": 0.25, "seed": 9}                       # the caller's dict is not consumed
    assert it.steps == [1, 2, 3, 1, 2, 3, 4, 5]                                  # the fit, epochs times over, then the held-out steps
    fit_x = [float(Batches.of([s])[0].sum()) for s in (1, 2, 3)]
    # the runner asked for ONCE, before any batch, and reset; per held-out batch: clean, apply + adv, control
    assert net.log == [("universal_runner", 4, 8), "reset"] + [("fit", s) for s in fit_x * 2] + ["forward", "apply", "forward", "forward"] * 2
    delta = torch.zeros(3, 8, 8)
    delta[0] = 0.1 * 6
    x, y = Batches.of([4, 5])
    g = torch.Generator().manual_seed(9)                                         # the control: drawn once from the seeded CPU generator
    if norm == "linf":
        control = (torch.randint(0, 2, (3, 8, 8), generator=g).float() * 2 - 1) * 0.25
        assert set(control.unique().tolist()) == {-0.25, 0.25}
    else:
        z = torch.randn(3, 8, 8, generator=g)
        control = z * (net.runner.delta.norm() / z.norm())
        assert float(control.norm()) == pytest.approx(float(delta.norm()), rel=1e-6)
    want = {"clean": p0(x), "adv": p0((x + net.runner.delta).clamp(-1, 1)), "control": p0((x + control).clamp(-1, 1))}
    assert set(got) == {"clean", "adv", "control", "attack"}
    for name in ("clean", "adv", "control"):
        same(got[name], expected(want[name], y))
    assert len(gathered) == 3 and all(torch.equal(a, want[k]) for a, k in zip(gathered, ("clean", "adv", "control")))
    a = got["attack"]
    assert set(a) == {"method", "norm", "eps", "steps", "clip", "delta", "linf", "l2", "fooled", "fooled_control", "fit_counted"}
    assert (a["method"], a["norm"], a["eps"], a["steps"]) == ("universal", norm, 0.25, 1)
    assert a["delta"].device.type == "cpu" and torch.equal(a["delta"], net.runner.delta) and torch.allclose(a["delta"], delta)
    assert a["linf"] == float(net.runner.delta.abs().max()) and a["l2"] == float(net.runner.delta.double().norm())
    assert a["fit_counted"] == [1, 2, 0, 1, 2, 0] and all(type(c) is int for c in a["fit_counted"])
    right = (want["clean"] < 0.5).long() == y
    for key, name in (("fooled", "adv"), ("fooled_control", "control")):
        flipped = ((want[name] < 0.5).long() != y) & right
        assert type(a[key]) is float and a[key] == float(flipped.sum()) / float(right.sum())
    assert 0 < int(right.sum()) < 8 and a["fooled"] > 0                          # the stub's shift flips some and not all


def test_stage_fooled_arithmetic_on_hand_made_scores(monkeypatch):
    """labels 0 (real: right where the score >= 0.5) and 1 (fake: right where it is < 0.5)"""
    scores = {"clean": torch.tensor([0.9, 0.8, 0.4, 0.7, 0.2, 0.1, 0.6, 0.3]),          # right: 0 1 3 | 4 5 7  (2 and 6 are wrong)
              "adv": torch.tensor([0.4, 0.8, 0.9, 0.3, 0.7, 0.1, 0.1, 0.6]),            # flips 0, 3, 4, 7 of the six
              "control": torch.tensor([0.9, 0.8, 0.9, 0.7, 0.2, 0.6, 0.6, 0.3])}        # flips 5
    labels = torch.tensor([0, 0, 0, 0, 1, 1, 1, 1])
    ev, net, it = make()
    monkeypatch.setattr(ev, "run", lambda n, body, first=1: {k: (v, labels) for k, v in scores.items()})
    a = ev.test_universal(2, 1, 1, {"eps": 0.25})["attack"]
    assert a["fooled"] == 4 / 6 and a["fooled_control"] == 1 / 6
    scores["clean"] = torch.tensor([0.1, 0.1, 0.1, 0.1, 0.9, 0.9, 0.9, 0.9])            # nothing classified correctly: NaN
    a = ev.test_universal(2, 1, 1, {"eps": 0.25})["attack"]
    assert a["fooled"] != a["fooled"] and a["fooled_control"] != a["fooled_control"]


def test_stage_refusals_fire_before_any_batch():
    ev, net, it = make()
    with pytest.raises(ValueError, match="^universal takes UniversalRunner's keyword arguments and 'seed': .*epz"):
        ev.test_universal(1, 1, 1, {"epz": 0.1})
    for kw, text in (({"batches": 0}, "batches must be an integer >= 1"), ({"fit_batches": 0}, "fit_batches must be an integer >= 1"),
                     ({"epochs": 1.5}, "epochs must be an integer >= 1")):
        with pytest.raises(ValueError, match=text):
            ev.test_universal(**dict({"batches": 1, "fit_batches": 1, "epochs": 1, "universal": {"eps": 0.1}}, **kw))
    assert it.steps == [] and "forward" not in net.log and net.runner is None
    # the real accessor's refusals are ValueErrors already: they pass through, before any batch
    ev = evaluate.Evaluator(_model(), _model(), it, 2, 8, DEV)
    with pytest.raises(ValueError, match="eps must be >= 0"):
        ev.test_universal(1, 1, 1, None)
    with pytest.raises(ValueError, match="universal takes UniversalRunner's keyword arguments and 'seed'"):
        ev.test_universal(1, 1, 1, {"eps": 0.1, "random_start": True})
    assert it.steps == []


def test_batches_first_argument_keeps_the_default():
    ev, net, it = make()
    assert [int(y.numel()) for _, y in ev.batches(2)] == [4, 4] and it.steps == [1, 2]
    del it.steps[:]
    list(ev.batches(3, first=4))
    assert it.steps == [4, 5, 6]
    assert list(evaluate.ROBUST) == ["pgd", "apgd", "square", "apgd+square", "fmn", "sparse_fmn"]      # the stage is no ROBUST method
