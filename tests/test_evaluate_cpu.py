"""engine/evaluate.py on the CPU: the stage rules of test / test_robust / test_corrupted / test_spatial against a stub model, a
seeded stub iterator and stub runners.  Every expected value is computed here from the stubs' outputs (metrics.cal_metrics
included), never taken from the evaluator."""
import re
import warnings

import numpy as np
import pytest
import torch

from unidefense_amd.engine import evaluate, metrics

DEV = torch.device("cpu")
GENERATOR = torch.Generator                           # the stubs' own, whatever a test puts in its place
EPS = 0.25                                            # exact in fp32: "radius == eps" and "one ulp above" are both representable
ABOVE = float(torch.nextafter(torch.tensor(EPS), torch.tensor(1.0)))


def logits(x):
    """two logits from per-sample means of two channel slices: raising channel 0 raises p(class 0)"""
    return torch.stack([x[:, :1].mean((1, 2, 3)), x[:, 1:].mean((1, 2, 3))], 1) * 8.0


def p0(x):
    return torch.softmax(logits(x), 1)[:, 0]


def shifted(x, delta):
    """x with channel 0 moved by delta (a number or one per sample)"""
    out = x.clone()
    out[:, 0] += torch.as_tensor(delta, dtype=x.dtype).reshape(-1, 1, 1)
    return out


class Batches:
    """seeded 4x3x8x8 batches (two real, two fake); fake_label=0 makes a single-class source, batch=0 an empty one"""

    def __init__(self, fake_label=1):
        self.fake_label, self.steps = fake_label, []

    def __call__(self, step, batch, size, device):
        self.steps.append(step)
        g = GENERATOR().manual_seed(100 + step)
        xr, xf = (torch.rand(batch, 3, size, size, generator=g) * 2 - 1 for _ in range(2))
        return (xr.to(device), torch.zeros(batch, dtype=torch.long, device=device),
                xf.to(device), torch.full((batch,), self.fake_label, dtype=torch.long, device=device))

    def all(self, batches, batch=2, size=8):
        parts = [Batches(self.fake_label)(s, batch, size, DEV) for s in range(1, batches + 1)]
        return torch.cat([torch.cat([p[0], p[2]]) for p in parts]), torch.cat([torch.cat([p[1], p[3]]) for p in parts])


class Runner:
    """A stub of every runner: .args = the accessor's kwargs (+ "method" as the real runners name themselves); a call logs
    itself and one draw of the generator it is handed, and returns x with channel 0 moved by `delta`.  `presets`: one dict of
    static results per call, copied into buffers the runner REUSES (as the real ones do; SpatialRunner's host-side `best`,
    which the stage copies to its device, is handed out fresh: on the CPU that copy is the identity)."""

    def __init__(self, net, name, kwargs, delta, presets=()):
        self.net, self.name, self.delta, self.presets, self.calls = net, name, delta, presets, 0
        self.args = dict(kwargs) if name == "pgd" else dict(kwargs, method=name)

    def __call__(self, x, y, *generator):
        assert len(generator) == (0 if self.name in ("pgd", "fmn", "sparse_fmn") else 1)      # who is handed a generator at all
        g = generator[0] if generator else None
        self.net.log.append(self.name)
        self.net.draws.append(None if g is None else (self.name, str(g.device), float(torch.rand(1, generator=g, device=g.device))))
        for k, v in (self.presets[self.calls % len(self.presets)] if self.presets else {}).items():
            if k == "best" or getattr(self, k, None) is None or getattr(self, k).shape != v.shape:
                setattr(self, k, torch.empty_like(v))
            getattr(self, k).copy_(v)
        self.calls += 1
        return shifted(x, self.delta)


class Net(torch.nn.Module):
    """forward(x) -> {"cls_out": logits(x)}; the accessors return (cached) stub runners; .log is the order of everything"""
    DELTA = {"pgd": 0.3, "apgd": [0.4, -0.4, 0.4, -0.4], "square": [-0.2, 0.2, -0.2, 0.2], "fmn": 0.5, "sparse_fmn": -0.5,
             "spatial": 0.1}

    def __init__(self, presets=None):
        super().__init__()
        self.log, self.draws, self.runners, self.presets = [], [], {}, presets or {}

    def forward(self, x):
        self.log.append("forward")
        return {"cls_out": logits(x)}

    def inference_runner(self, n, size, precision):
        self.log.append(("inference_runner", n, size, precision))
        return lambda x: {"cls_out": logits(x)}

    def _runner(self, name, n, size, kwargs):
        self.log.append(("attack_runner" if name == "pgd" else name + "_runner", n, size))
        if name not in self.runners:
            self.runners[name] = Runner(self, name, kwargs, self.DELTA[name], self.presets.get(name, ()))
        return self.runners[name]

    def attack_runner(self, n, size, **kw):
        return self._runner("pgd", n, size, kw)

    def apgd_runner(self, n, size, **kw):
        return self._runner("apgd", n, size, kw)

    def square_runner(self, n, size, **kw):
        return self._runner("square", n, size, kw)

    def fmn_runner(self, n, size, **kw):
        return self._runner("fmn", n, size, kw)

    def sparse_fmn_runner(self, n, size, **kw):
        return self._runner("sparse_fmn", n, size, kw)

    def spatial_runner(self, n, size, grid=(3, 2, 1), search="grid"):
        return self._runner("spatial", n, size, {"grid": grid, "search": search})


def make(net=None, it=None, batch=2, device=DEV, **kw):
    net, it = net or Net(), it or Batches()
    return evaluate.Evaluator(net, net, it, batch, 8, device, **kw), net, it


def expected(scores, labels):
    """what test() returns for (scores, labels), by the definitions"""
    sc, lb = scores.numpy(), labels.numpy()
    ret = {"scores": scores, "labels": labels, "acc": float(np.mean((sc < 0.5).astype(int) == lb))}
    if len(set(lb.tolist())) == 2:
        ret.update(metrics.cal_metrics(lb, sc, threshold=0.5))
    return ret


def same(got, want):
    assert set(got) == set(want)
    for k, v in want.items():
        assert torch.equal(got[k], v) if torch.is_tensor(v) else got[k] == v, k
    assert got["scores"].device.type == "cpu" and got["labels"].dtype == torch.int64


def line(tag, r):
    return "%s | EER %.4f, HTER %.4f, TPR 5%% %.4f, AUC %.4f, ACC %.4f\n" % (tag, r["EER"], r["ACER"], r["TPR5%"], r["AUC"], r["ACC"])


# ---- test() and the scoring forward ----------------------------------------------------------------------------------------------
def test_test_is_the_direct_computation(capsys):
    ev, net, it = make()
    got = ev.test(3)
    x, y = it.all(3)
    want = expected(p0(x), y)
    same(got, want)
    assert {"AUC", "EER", "ACER", "TPR5%", "ACC", "NumP", "NumN"} <= set(got) and got["NumP"] == got["NumN"] == 6
    assert capsys.readouterr().out == line("Test", want)                     # the line, byte for byte
    assert it.steps == [1, 2, 3] and net.log == ["forward"] * 3
    make(local_rank=1)[0].test(3)
    assert capsys.readouterr().out == ""                                      # only rank 0 prints


def test_single_class_source_has_no_roc_keys_and_prints_nothing(capsys):
    ev, _, it = make(it=Batches(fake_label=0))
    got = ev.test(2)
    x, y = it.all(2)
    same(got, expected(p0(x), y))
    assert set(got) == {"scores", "labels", "acc"} and capsys.readouterr().out == ""


def test_inference_graph_selects_the_forward():
    ev, net, _ = make(inference_graph=True, inference_precision="fp16")
    graphed = ev.test(2)
    assert net.log == [("inference_runner", 4, 8, "fp16")] * 2                # never model(x)
    ev, net, _ = make()
    same(ev.test(2), graphed)
    assert net.log == ["forward"] * 2                                         # never the runner
    ev, net, _ = make(inference_graph=True)
    ev.test_robust(1, {"eps": 0.1})
    assert net.log == [("inference_runner", 4, 8, "fp32"), ("attack_runner", 4, 8), "pgd", ("inference_runner", 4, 8, "fp32")]


# ---- test_robust: pgd, apgd, square and the ensemble --------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["pgd", "apgd", "square"])
def test_robust_scores_the_runners_output(method, capsys):
    ev, net, it = make()
    attack = {"eps": 0.1, "steps": 3, "method": method}
    got = ev.test_robust(2, attack if method != "pgd" else {"eps": 0.1, "steps": 3})
    assert attack == {"eps": 0.1, "steps": 3, "method": method}               # the caller's dict is not consumed
    x, y = it.all(2)
    delta = torch.as_tensor(Net.DELTA[method]).expand(2, -1).reshape(-1) if method != "pgd" else Net.DELTA[method]
    clean, adv = expected(p0(x), y), expected(p0(shifted(x, delta)), y)
    assert set(got) == {"clean", "adv", "attack"}
    same(got["clean"], clean)
    same(got["adv"], adv)
    assert capsys.readouterr().out == line("Test", clean) + line("Test(adv)", adv)
    # "attack" is the runner's own dictionary: no "method" for pgd, the runner's "method" otherwise
    assert got["attack"] == ({"eps": 0.1, "steps": 3} if method == "pgd" else {"eps": 0.1, "steps": 3, "method": method})
    # per batch: the clean score, THEN the accessor, the attack and its score
    accessor = {"pgd": "attack_runner"}.get(method, method + "_runner")
    assert net.log == ["forward", (accessor, 4, 8), method, "forward"] * 2
    assert net.draws == [None] * 2                                            # no seed: no generator (None is handed over)


def test_robust_ensemble_keeps_the_worst_case_per_sample():
    ev, net, it = make()
    ap, sq = {"eps": 0.1, "steps": 3}, {"eps": 0.2, "steps": 4}
    both = {"method": "apgd+square", "apgd": ap, "square": sq, "seed": 3}
    got = ev.test_robust(2, both)
    assert both == {"method": "apgd+square", "apgd": ap, "square": sq, "seed": 3}
    x, y = it.all(2)
    s = p0(shifted(x, torch.tensor(Net.DELTA["apgd"]).repeat(2)))
    s2 = p0(shifted(x, torch.tensor(Net.DELTA["square"]).repeat(2)))
    want = torch.stack([(min if int(t) == 0 else max)(float(a), float(b)) * torch.ones(()) for a, b, t in zip(s, s2, y)])
    # the stub pair makes every case occur: both classes, and in each class both members win
    for cls in (0, 1):
        assert {bool(w == a) for w, a, t in zip(want, s, y) if int(t) == cls} == {True, False}
    assert torch.equal(got["adv"]["scores"], want)
    same(got["clean"], expected(p0(x), y))
    same(got["adv"], expected(want, y))
    assert got["attack"] == {"method": "apgd+square", "apgd": dict(ap, method="apgd"), "square": dict(sq, method="square")}
    # Auto-PGD runs and is scored before Square; the clean score comes first
    assert net.log == ["forward", ("apgd_runner", 4, 8), "apgd", "forward", ("square_runner", 4, 8), "square", "forward"] * 2
    alone = [make()[0].test_robust(2, dict(d, method=m, seed=3))["adv"]["scores"] for m, d in (("apgd", ap), ("square", sq))]
    assert torch.equal(alone[0], s) and torch.equal(alone[1], s2)             # the members, composed and not re-implemented


def test_seeds_and_generators(monkeypatch):
    made = []
    real = torch.Generator

    def recording(device="cpu"):
        made.append(device)
        return real(device=device)

    monkeypatch.setattr(torch, "Generator", recording)
    dev = torch.device("cpu", 0)                       # tells "the evaluator's device" from "the CPU" on a machine without a GPU
    runs = {}
    for method, attack in (("apgd", {"eps": 0.1}), ("square", {"eps": 0.1}), ("apgd+square", {"apgd": {"eps": 0.1}, "square": {}})):
        for rep in range(2):
            ev, net, _ = make(device=dev)
            del made[:]
            ev.test_robust(2, dict(attack, method=method, seed=7))
            runs[method, rep] = net.draws
            # Auto-PGD's generator on the evaluator's device, Square's on the CPU — one of each per call, from the one seed
            assert [str(d) for d in made] == {"apgd": ["cpu:0"], "square": ["cpu"], "apgd+square": ["cpu:0", "cpu"]}[method]
            assert all("seed" not in r.args for r in net.runners.values())    # "seed" is popped before a runner sees the dict
        assert runs[method, 0] == runs[method, 1] and all(d is not None for d in runs[method, 0])
        assert len({d[2] for d in runs[method, 0] if d[0] == method.split("+")[0]}) == 2      # one generator, consumed across batches
    want = real().manual_seed(7)
    assert [d[2] for d in runs["square", 0]] == [float(torch.rand(1, generator=want)) for _ in range(2)]
    assert [d for d in runs["apgd+square", 0] if d[0] == "square"] == runs["square", 0]
    # "pgd" never pops "seed": it reaches the runner's arguments (where AttackRunner refuses it)
    ev, net, _ = make(device=dev)
    del made[:]
    res = ev.test_robust(1, {"eps": 0.1, "seed": 7})
    assert res["attack"] == {"eps": 0.1, "seed": 7} and made == [] and net.draws == [None]


# ---- fmn / sparse_fmn ------------------------------------------------------------------------------------------------------------------
FMN = [{"found": torch.tensor([1, 0, 1, 1], dtype=torch.uint8), "radius": torch.tensor([EPS, 0.1, ABOVE, 0.1])},
       {"found": torch.tensor([0, 1, 1, 1], dtype=torch.uint8), "radius": torch.tensor([0.1, 0.2, 0.3, 0.05])}]


@pytest.mark.parametrize("method", ["fmn", "sparse_fmn"])
@pytest.mark.parametrize("eps", [EPS, None])
def test_robust_min_norm_take_rule(method, eps):
    ev, net, it = make(net=Net({method: FMN}))
    attack = {"method": method, "steps": 5} if eps is None else {"method": method, "steps": 5, "eps": eps}
    got = ev.test_robust(2, attack)
    x, y = it.all(2)
    found, radius = torch.cat([p["found"] for p in FMN]), torch.cat([p["radius"] for p in FMN])
    take = [bool(f) and (eps is None or float(r) <= eps) for f, r in zip(found, radius)]
    assert take == ([True, False, False, True, False, True, False, True] if eps is not None else [bool(f) for f in found])
    xa = shifted(x, Net.DELTA[method])
    scored = torch.stack([xa[i] if t else x[i] for i, t in enumerate(take)])  # x_adv or x, sample by sample
    same(got["clean"], expected(p0(x), y))
    same(got["adv"], expected(p0(scored), y))
    a = got["attack"]
    assert {k: v for k, v in a.items() if k not in ("radius", "found")} == {
        "steps": 5, "method": method, "eps": eps, "median_radius": float(radius.double().median())}
    assert (a["eps"] is None or type(a["eps"]) is float) and type(a["median_radius"]) is float
    # cloned per batch (the runner reuses its buffers) and gathered: both batches' values, as CPU float32 / int32
    assert a["radius"].dtype == torch.float32 and a["radius"].device.type == "cpu" and torch.equal(a["radius"], radius)
    assert a["found"].dtype == torch.int32 and a["found"].device.type == "cpu" and torch.equal(a["found"], found.int())
    assert net.log == ["forward", (method + "_runner", 4, 8), method, "forward"] * 2
    assert "eps" not in net.runners[method].args or net.runners[method].args["eps"] is None


def test_robust_min_norm_empty_radius_gives_nan_median():
    empty = [{"found": torch.zeros(0, dtype=torch.uint8), "radius": torch.zeros(0)}]
    ev, _, _ = make(net=Net({"fmn": empty}), batch=0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                 # numpy's mean of an empty slice, in "acc"
        a = ev.test_robust(1, {"method": "fmn"})["attack"]
    assert a["radius"].numel() == 0 and a["median_radius"] != a["median_radius"]


# ---- test_corrupted with a host stand-in -----------------------------------------------------------------------------------------------
def stand_in(calls):
    def corrupt(x, kind, level, generator=None, subsampling="420", out=None):
        draw = None if generator is None else float(torch.rand(1, generator=generator, device=generator.device))
        calls.append((float(x.sum()), kind, level, subsampling, out, draw))
        return out.copy_(x * (0.5 if kind == "jpeg" else -1.0) / level)
    return corrupt


def test_corrupted_keys_order_buffer_and_means(monkeypatch, capsys):
    # the gather of ("jpeg", 3) — the third of five — hands back single-class labels, as ranks without fakes would
    n = [0]

    def gather(scores, labels):
        n[0] += 1
        return scores, torch.zeros_like(labels) if n[0] == 3 else labels

    monkeypatch.setattr(metrics, "gather_scores", gather)
    calls = []
    ev, net, it = make()
    got = ev.test_corrupted(2, ["jpeg", "gaussian_noise"], (1, 3), 5, "444", corrupt=stand_in(calls))
    x, y = it.all(2)
    assert set(got) == {"clean", "corrupted", "mean", "corruptions"}
    assert list(got["corrupted"]) == ["jpeg", "gaussian_noise"] and all(list(v) == [1, 3] for v in got["corrupted"].values())
    from unidefense_amd import corrupt as CR
    assert got["corruptions"] == {k: {lv: CR.LEVELS[k][lv - 1] for lv in (1, 3)} for k in ("jpeg", "gaussian_noise")}
    same(got["clean"], expected(p0(x), y))
    want = {(k, lv): expected(p0(x * f / lv), torch.zeros_like(y) if (k, lv) == ("jpeg", 3) else y)
            for k, f in (("jpeg", 0.5), ("gaussian_noise", -1.0)) for lv in (1, 3)}
    for (k, lv), w in want.items():
        same(got["corrupted"][k][lv], w)
    # the mean covers only the levels that have both classes
    assert "AUC" not in got["corrupted"]["jpeg"][3]
    noise = [want["gaussian_noise", lv] for lv in (1, 3)]
    assert got["mean"] == {"jpeg": {m: float(want["jpeg", 1][m]) for m in ("AUC", "ACC")},
                           "gaussian_noise": {m: float(sum(r[m] for r in noise) / 2) for m in ("AUC", "ACC")}}
    out = capsys.readouterr().out.splitlines()
    assert [ln.split(" |")[0].split()[0] for ln in out] == ["Test", "Test(jpeg", "Corrupted", "Test(gaussian_noise", "Test(gaussian_noise",
                                                            "Corrupted"]
    assert out[2] == "Corrupted %-14s | mean AUC %.4f, mean ACC %.4f | AUC by level 1:%.4f" % (
        "jpeg", got["mean"]["jpeg"]["AUC"], got["mean"]["jpeg"]["ACC"], want["jpeg", 1]["AUC"])
    # batch-major, then (kind, level) in insertion order; every call writes the one x_cor buffer; one generator for all
    sums = [float(x[:4].sum()), float(x[4:].sum())]
    assert [c[:4] for c in calls] == [(s, k, lv, "444") for s in sums for k in ("jpeg", "gaussian_noise") for lv in (1, 3)]
    assert all(c[4] is calls[0][4] for c in calls) and calls[0][4].shape == (4, 3, 8, 8)
    g = torch.Generator().manual_seed(5)
    assert [c[5] for c in calls] == [float(torch.rand(1, generator=g)) for _ in range(8)]
    assert net.log == ["forward"] * 10
    # no seed: no generator; no kinds: all of corrupt.CORRUPTIONS
    del calls[:]
    got = make()[0].test_corrupted(1, None, (2,), None, "420", corrupt=stand_in(calls))
    assert list(got["corrupted"]) == list(CR.CORRUPTIONS) and all(c[5] is None for c in calls) and len(calls) == 7


# ---- test_spatial ----------------------------------------------------------------------------------------------------------------------
def spatial_presets(loss0):
    best = torch.arange(20.0, dtype=torch.float64).reshape(4, 5)
    return [{"best": best, "best_loss": torch.tensor([-0.5, -2.0, 0.5, 0.0]), "loss0": torch.tensor(loss0)},
            {"best": best + 100, "best_loss": torch.tensor([1.0, 1.0, -1.0, 1.0]), "loss0": torch.tensor(loss0)}]


def test_spatial_best_fooled_and_order():
    ev, net, it = make(net=Net({"spatial": spatial_presets([1.0, -1.0, 2.0, 3.0])}))
    got = ev.test_spatial(2, {"grid": (5, 1, 1), "seed": 4})
    x, y = it.all(2)
    same(got["clean"], expected(p0(x), y))
    same(got["adv"], expected(p0(shifted(x, Net.DELTA["spatial"])), y))
    a = got["attack"]
    assert set(a) == {"grid", "search", "method", "best", "fooled"} and a["grid"] == (5, 1, 1) and a["method"] == "spatial"
    best = torch.arange(20.0, dtype=torch.float64).reshape(4, 5)
    assert a["best"].device.type == "cpu" and a["best"].shape == (8, 5) and torch.equal(a["best"], torch.cat([best, best + 100]))
    # held (loss0 > 0): samples 0, 2, 3 of each batch; best_loss <= 0 among them: 0 and 3 of the first batch, 2 of the second
    assert a["fooled"] == 3 / 6 and type(a["fooled"]) is float
    # the runner BEFORE the clean score; one CPU generator per call, consumed across the batches
    assert net.log == [("spatial_runner", 4, 8), "forward", "spatial", "forward"] * 2
    g = torch.Generator().manual_seed(4)
    assert net.draws == [("spatial", "cpu", float(torch.rand(1, generator=g))) for _ in range(2)]
    ev, net, _ = make(net=Net({"spatial": spatial_presets([0.0, -1.0, -2.0, 0.0])}))
    a = ev.test_spatial(1, None)["attack"]
    assert a["fooled"] != a["fooled"] and a["grid"] == (3, 2, 1) and net.draws == [None]    # nothing held: NaN; no seed: no generator


def test_spatial_unknown_key_is_a_value_error_of_the_accessor_only():
    ev, net, it = make()
    with pytest.raises(ValueError, match="^spatial takes SpatialRunner's keyword arguments and 'seed': .*max_angel"):
        ev.test_spatial(1, {"max_angel": 3.0})
    assert net.log == []                                # raised by the accessor, before any forward

    def broken(x, y, generator):
        raise TypeError("inside the search")

    net.runners["spatial"] = broken
    with pytest.raises(TypeError, match="inside the search"):                 # a TypeError of the run itself stays one
        ev.test_spatial(1, None)


# ---- refusals: all ValueError, with today's text, before any stub is touched ----------------------------------------------------------
def test_refusals_fire_before_anything_runs():
    calls = []
    ev, net, it = make()
    corrupted = lambda *a, **kw: ev.test_corrupted(1, *a, corrupt=stand_in(calls), **kw)          # noqa: E731
    cases = [
        (lambda: ev.test_robust(1, None), "test_robust needs an attack: pass attack={...} or set config['config']['attack']"),
        (lambda: ev.test_robust(1, {}), "test_robust needs an attack"),
        (lambda: ev.test_robust(1, {"method": "spatial", "eps": 0.1}),
         "attack method must be 'pgd', 'apgd', 'square', 'apgd+square', 'fmn' or 'sparse_fmn', got 'spatial'"),
        (lambda: ev.test_robust(1, {"method": "apgd+square", "eps": 0.1, "seed": 1}),
         "attack method 'apgd+square' takes {'apgd': {...}, 'square': {...}, 'seed': ...}, got the keys ['eps']"),
        (lambda: ev.test_robust(1, {"method": "apgd+square", "apgd": {}}), "got the keys ['apgd']"),
        (lambda: ev.test_robust(1, {"method": "apgd+square", "apgd": {}, "square": {}, "eps": 1}), "got the keys ['apgd', 'eps', 'square']"),
        (lambda: ev.test_robust(1, {"method": "fmn", "eps": -0.5}), "eps must be >= 0, got -0.5"),
        (lambda: ev.test_robust(1, {"method": "sparse_fmn", "eps": float("nan")}), "eps must be >= 0, got nan"),
        (lambda: corrupted(["jpeg"], (1,), None, "411"), "subsampling must be one of ('420', '444'), got '411'"),
        (lambda: corrupted(["fog"], (1,), None, "420"), "fog"),                      # corrupt.resolve's own
        (lambda: corrupted(["jpeg"], (6,), None, "420"), "level"),
    ]
    for call, text in cases:
        with pytest.raises(ValueError, match=re.escape(text)):
            call()
        assert net.log == [] and net.runners == {} and it.steps == [] and calls == []
    assert list(evaluate.ROBUST) == ["pgd", "apgd", "square", "apgd+square", "fmn", "sparse_fmn"]      # names and message: one table


# ---- collectives: gather_scores calls per stage at world size 1 -----------------------------------------------------------------------
def test_gather_scores_calls_per_stage(monkeypatch):
    seen = []
    real = metrics.gather_scores
    monkeypatch.setattr(metrics, "gather_scores", lambda s, lb: seen.append(s) or real(s, lb))
    presets = {"fmn": FMN, "sparse_fmn": FMN, "spatial": spatial_presets([1.0, 1.0, 1.0, 1.0])}

    def count(stage):
        del seen[:]
        stage(make(net=Net(presets))[0])
        assert all(s.shape == (8,) for s in seen)                             # always one 1-D column of all batches
        return len(seen)

    assert count(lambda ev: ev.test(2)) == 1                                  # test(): the scores
    for method in ("pgd", "apgd", "square"):
        assert count(lambda ev: ev.test_robust(2, {"method": method, "eps": 0.1})) == 2        # clean, adv
    assert count(lambda ev: ev.test_robust(2, {"method": "apgd+square", "apgd": {}, "square": {}})) == 2      # clean, merged adv
    for method in ("fmn", "sparse_fmn"):
        assert count(lambda ev: ev.test_robust(2, {"method": method})) == 4   # radius, found, clean, adv — in this order
        assert torch.equal(seen[0], torch.cat([p["radius"] for p in FMN])) and torch.equal(seen[1], torch.cat([p["found"] for p in FMN]))
        assert seen[2].dtype == seen[3].dtype == torch.float32 and not torch.equal(seen[2], seen[3])
    # test_corrupted: clean + one per (kind, level): 1 + 2 * 3
    assert count(lambda ev: ev.test_corrupted(2, ["jpeg", "block"], (1, 2, 3), None, "420", corrupt=stand_in([]))) == 7
    assert count(lambda ev: ev.test_spatial(2, None)) == 9                    # best's five columns, best_loss, loss0, clean, adv
    want = spatial_presets([1.0, 1.0, 1.0, 1.0])
    assert all(torch.equal(seen[i], torch.cat([p["best"][:, i] for p in want])) for i in range(5))
    assert torch.equal(seen[5], torch.cat([p["best_loss"] for p in want])) and torch.equal(seen[6], torch.ones(8))


def test_the_module_loads_nothing_native():
    import ast
    import inspect
    tree = ast.parse(inspect.getsource(evaluate))
    top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
    names = {a.name for n in top for a in n.names} | {n.module for n in top if isinstance(n, ast.ImportFrom)}
    assert names == {"partial", "functools", "torch", "metrics", None}        # no lib / kernels / attack / corrupt at import time
