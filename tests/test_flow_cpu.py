"""CPU: the flow-field attack's host side (unidefense_amd/flow.py, engine/evaluate.py: test_flow): the float64 restatements
against torch's grid_sample and autograd, every refusal without a device, the four entry points' argument tests, the header's
rows, the runner cache's key and the stage's rules against stubs."""
import ctypes
import math
import re

import pytest
import torch
import torch.nn.functional as F

from tests.margins import within
from unidefense_amd import flow as FL
from unidefense_amd.engine import evaluate

BOUND = 2.0
KINDS = ("zero", "integer", "small", "large", "bound", "half")


def make_flow(kind, n, S, seed, bound=BOUND):
    """the flow kinds of the suite, fp32 [n, 2, S, S] in pixels"""
    g = torch.Generator().manual_seed(seed)
    if kind == "zero":
        return torch.zeros(n, 2, S, S)
    if kind == "integer":
        return torch.randint(-3, 4, (n, 2, S, S), generator=g).float()
    if kind == "small":
        return torch.randn(n, 2, S, S, generator=g) * 0.7
    if kind == "large":
        return torch.randn(n, 2, S, S, generator=g) * float(S)
    if kind == "bound":                                           # every component exactly at +-bound
        return (torch.randint(0, 2, (n, 2, S, S), generator=g).float() * 2 - 1) * bound
    if kind == "half":                                            # half-integers: the fraction is exactly 1/2
        return torch.randint(-3, 4, (n, 2, S, S), generator=g).float() + 0.5
    raise KeyError(kind)


def make_images(n, S, seed):
    return torch.randn(n, 3, S, S, generator=torch.Generator().manual_seed(seed))


def torch_warp(x, w):
    """float64 grid_sample(bilinear, border, align_corners=True) at grid = 2 q / (S - 1) - 1, q the fp32 coordinate"""
    S = x.shape[-1]
    idx = torch.arange(S, dtype=torch.float32)
    qx = (idx.view(1, 1, S) + w[:, 0]).double()                   # ONE fp32 rounding, as the kernels
    qy = (idx.view(1, S, 1) + w[:, 1]).double()
    grid = torch.stack([2.0 * qx / (S - 1) - 1.0, 2.0 * qy / (S - 1) - 1.0], -1)
    return F.grid_sample(x.double(), grid, mode="bilinear", padding_mode="border", align_corners=True), qx, qy


# ---- the restatements against torch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S", [2, 5, 8, 33])
def test_ref_warp_and_grad_against_grid_sample(S, kind):
    n = 2
    x, w, g = make_images(n, S, 1), make_flow(kind, n, S, 2), make_images(n, S, 3).double()
    want, _, _ = torch_warp(x, w)
    got = FL.ref_flow_warp(x, w)
    assert got.dtype == torch.float64
    mx = float(x.abs().max())
    assert within("ref warp vs grid_sample", (got - want).abs().max() / mx, 1e-12)
    # the gradient: autograd through grid_sample with respect to the coordinate, q = index + w so d/dw = d/dq
    wq = w.double().clone().requires_grad_()
    q32x = (torch.arange(S, dtype=torch.float32).view(1, 1, S) + w[:, 0]).double()
    q32y = (torch.arange(S, dtype=torch.float32).view(1, S, 1) + w[:, 1]).double()
    # the same fp32 coordinate, as a differentiable function of wq with slope 1
    qx = q32x + (wq[:, 0] - wq[:, 0].detach())
    qy = q32y + (wq[:, 1] - wq[:, 1].detach())
    grid = torch.stack([2.0 * qx / (S - 1) - 1.0, 2.0 * qy / (S - 1) - 1.0], -1)
    out = F.grid_sample(x.double(), grid, mode="bilinear", padding_mode="border", align_corners=True)
    gw, = torch.autograd.grad((out * g).sum(), wq)
    got = FL.ref_flow_grad(g, x, w)
    scale = g.abs().sum(1, keepdim=True) * mx
    assert within("ref grad vs autograd", ((got - gw).abs() / scale).max(), 1e-12)
    if kind in ("bound", "large"):                                # clamped coordinates have a zero gradient: some exist here
        inside = (q32x > 0) & (q32x < S - 1)
        assert bool((got[:, 0][~inside] == 0).all()) and bool((~inside).any())


@pytest.mark.parametrize("S", [2, 5, 8])
def test_ref_tv_gradient_against_autograd(S):
    eps = 1e-8
    for kind in ("zero", "small", "integer"):
        w = make_flow(kind, 2, S, 4).double().requires_grad_()
        dh, dv = w[:, :, :, 1:] - w[:, :, :, :-1], w[:, :, 1:, :] - w[:, :, :-1, :]
        loss = torch.sqrt((dh * dh).sum(1) + eps).flatten(1).sum(1) + torch.sqrt((dv * dv).sum(1) + eps).flatten(1).sum(1)
        want, = torch.autograd.grad(loss.sum(), w)
        val, got = FL.ref_flow_tv(w.detach(), eps)
        assert within("ref tv value", (val - loss.detach()).abs().max() / loss.detach().abs().max(), 1e-12)
        assert within("ref tv gradient", (got - want).abs().max(), 1e-12 * 4)            # at most four terms of magnitude <= 1
        if kind == "zero":
            assert bool((got == 0).all())
            assert val.tolist() == pytest.approx([2 * S * (S - 1) * 1e-4] * 2, rel=1e-12)


def test_zero_flow_returns_the_input_and_an_integer_flow_shifts():
    x = make_images(2, 9, 5)
    assert torch.equal(FL.ref_flow_warp(x, torch.zeros(2, 2, 9, 9)), x.double())
    w = torch.zeros(2, 2, 9, 9)
    w[:, 0], w[:, 1] = 2.0, -1.0                                  # out(r, c) = x(r - 1, c + 2)
    got = FL.ref_flow_warp(x, w)
    assert torch.equal(got[:, :, 1:, :7], x.double()[:, :, :8, 2:])
    assert torch.equal(got[:, :, 0, :7], x.double()[:, :, 0, 2:])                       # the border: the clamped row
    # a NaN component: NaN at that pixel only; +-inf and huge values: a border pixel
    w = torch.zeros(1, 2, 9, 9)
    w[0, 0, 3, 4], w[0, 1, 5, 5], w[0, 0, 1, 1], w[0, 1, 2, 2] = float("nan"), float("inf"), -float("inf"), 1e30
    got = FL.ref_flow_warp(x[:1], w)
    nan = torch.isnan(got)
    assert bool(nan[0, :, 3, 4].all()) and int(nan.sum()) == 3
    assert torch.equal(got[0, :, 5, 5], x[0, :, 8, 5].double()) and torch.equal(got[0, :, 1, 1], x[0, :, 1, 0].double())
    assert torch.equal(got[0, :, 2, 2], x[0, :, 8, 2].double())


def test_ref_control_table():
    nan = float("nan")
    # per sample over k = 0..4:        ties,           a NaN at k = 0,        a NaN later,          a strict climb
    table = torch.tensor([[1.0, 1.0, 0.5, 1.0, 2.0], [nan, 0.3, 0.2, nan, 0.4], [0.5, nan, 0.7, 0.7, 0.1], [0.1, 0.2, 0.3, 0.4, 0.5]]).t()
    for maximise, keeps, bests in ((True, [[1, 0, 0, 0, 1], [1, 1, 0, 0, 1], [1, 0, 1, 0, 0], [1, 1, 1, 1, 1]], [2.0, 0.4, 0.7, 0.5]),
                                   (False, [[1, 0, 1, 0, 0], [1, 1, 1, 0, 0], [1, 0, 0, 0, 1], [1, 0, 0, 0, 0]], [0.5, 0.2, 0.1, 0.1])):
        best = torch.zeros(4, dtype=torch.float64)
        got = []
        for k in range(5):
            keep, best = FL.ref_flow_control(table[k], k, best, maximise)
            got.append(keep.long().tolist())
        assert torch.tensor(got).t().tolist() == keeps, maximise
        assert best.tolist() == pytest.approx(bests)


def test_ref_update_on_hand_values():
    w = torch.tensor([0.0, 1.9, -1.9, 0.3, 0.3, 0.5]).view(1, 2, 1, 3).repeat(2, 1, 1, 1)
    gw = torch.tensor([1.0, 2.0, -3.0, 0.0, -0.0, float("nan")]).view(1, 2, 1, 3).repeat(2, 1, 1, 1)
    wb = torch.full_like(w, 7.0)
    new, best = FL.ref_flow_update(w, wb, gw, torch.tensor([1, 0]), 0.25, 2.0)
    assert new.dtype == torch.float64
    flat = new[0].flatten().tolist()
    assert flat[:5] == [0.25, 2.0, -2.0, float(w.flatten()[3]), float(w.flatten()[4])] and math.isnan(flat[5])
    assert torch.equal(best[0], w[0].double()) and torch.equal(best[1], wb[1].double())


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _model():
    from unidefense_amd.model import load_model
    return load_model("UDR18")(num_classes=2).eval()


BAD = [({"max_flow": -1.0}, "max_flow must be a finite number >= 0"), ({"max_flow": float("nan")}, "max_flow must be a finite"),
       ({"max_flow": float("inf")}, "max_flow must be a finite"), ({"max_flow": None}, "max_flow must be a finite"),
       ({"tau": -0.1}, "tau must be a finite number >= 0"), ({"tau": float("inf")}, "tau must be a finite"),
       ({"tau": float("nan")}, "tau must be a finite"), ({"tv_eps": 0.0}, "tv_eps must be a finite number > 0"),
       ({"tv_eps": -1e-8}, "tv_eps must be"), ({"tv_eps": float("nan")}, "tv_eps must be"), ({"steps": 0}, "steps must be an integer >= 1"),
       ({"steps": 2.5}, "steps must be an integer >= 1"), ({"step": float("nan")}, "step must be a number"),
       ({"objective": "margin"}, "objective must be 'cross_entropy' or a callable"),
       ({"precision": "bf16"}, "precision"), ({"precision": "fp16"}, "fp16"), ({"grad_scale": 3.0}, "grad_scale")]


@pytest.mark.parametrize("kw,text", BAD)
def test_refusals_need_no_device(kw, text):
    m = _model()
    for make in (lambda: FL.FlowRunner(m, 2, 64, **kw), lambda: FL.flow_runner(m, 2, 64, **kw), lambda: m.flow_runner(2, 64, **kw)):
        with pytest.raises(ValueError, match=re.escape(text)):
            make()
    assert not m.__dict__.get("_ud_flow_runners")


def test_host_side_refusals():
    from unidefense_amd.attack import resolve_step
    from unidefense_amd.model import load_model
    m = load_model("UDR18")(num_classes=2)
    with pytest.raises(ValueError, match="size must be an integer >= 2"):
        FL.FlowRunner(m.eval(), 2, 1)
    with pytest.raises(ValueError, match="eval"):
        FL.FlowRunner(m.train(), 2, 64)
    with pytest.raises(ValueError, match="cuda"):                 # every argument passed: only the device is missing
        FL.FlowRunner(m.eval(), 2, 64, max_flow=1.5, steps=3, step=0.5, tau=0.0, tv_eps=1e-6, targeted=True,
                      objective=lambda out, y: out["cls_out"][:, 0])
    with pytest.raises(ValueError, match="takes a UDEB4"):
        FL.FlowRunner(torch.nn.Linear(2, 2), 2, 64)
    for name in ("UDEB4", "UDR18", "UDR50"):
        assert callable(getattr(load_model(name), "flow_runner"))
    a = FL._flow_arguments(4, 128)
    assert list(a) == ["batch", "size", "max_flow", "steps", "step", "tau", "tv_eps", "targeted", "objective", "precision", "grad_scale"]
    assert tuple(a.values())[2:] == (2.0, 20, None, 0.05, 1e-8, False, "cross_entropy", "fp32", None)
    assert resolve_step(2.0, 20) == 0.25                          # step=None: the PGD rule on max_flow
    # flow_warp: corrupt._check_images' refusals, then the flow's
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(ValueError, match="flow_warp takes a cuda tensor"):
        FL.flow_warp(x, torch.zeros(2, 2, 8, 8))
    with pytest.raises(ValueError, match="flow_warp takes a cuda tensor"):
        FL.flow_warp([1.0], None)


def test_wrappers_refuse_cpu_tensors_and_bad_arguments_before_any_hip_call():
    from unidefense_amd import kernels as K
    x, w = torch.zeros(2, 3, 4, 4), torch.zeros(2, 2, 4, 4)
    keep = torch.zeros(2, dtype=torch.int32)
    ist, fst, hist = torch.zeros(2, 2, dtype=torch.int32), torch.zeros(1, 2), torch.zeros(4, 2)
    for call in (lambda: K.flow_warp(x, w, x.clone()), lambda: K.flow_grad(x.clone(), x, w, w.clone()),
                 lambda: K.flow_control(torch.zeros(2), ist, fst, hist),
                 lambda: K.flow_update(w, w.clone(), w.clone(), keep, x, x.clone(), 0.1, 2.0),
                 lambda: K.flow_state(2, 3, torch.device("cpu")) and K.flow_control(torch.zeros(2), *K.flow_state(2, 3, torch.device("cpu")))):
        with pytest.raises(ValueError, match="CUDA"):
            call()
    assert [tuple(t.shape) for t in K.flow_state(3, 5, torch.device("cpu"))] == [(2, 3), (1, 3), (6, 3)]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_refuse_bad_arguments():
    from tests.test_abi_cpu import header
    from unidefense_amd import kernels as K
    from unidefense_amd import lib
    h = header()
    L = ctypes.CDLL(lib.LIB_PATH)
    names = ("ud_flow_warp", "ud_flow_grad", "ud_flow_control", "ud_flow_update")
    assert [n for n in h.protos if n.startswith("ud_flow")] == list(names)
    for n in names:
        assert n in lib.EXPORTED and hasattr(L, n), n
        assert h.protos[n][0] is ctypes.c_int, n
        fn = getattr(L, n)
        fn.restype, fn.argtypes = ctypes.c_int, [t for t, _ in h.protos[n][1]]
    for n in ("flow_state", "flow_warp", "flow_grad", "flow_control", "flow_update"):
        assert callable(getattr(K, n)), n
    rows = {k[len("UD_FLOW_I_"):].lower(): v for k, v in h.consts.items() if k.startswith("UD_FLOW_I_")}
    assert K.FLOW_I == rows == {"k": 0, "keep": 1}
    assert K.FLOW_F == {"f_best": 0} and h.consts["UD_FLOW_F_BEST"] == 0
    buf = (ctypes.c_double * 64)()
    a, b, c, d, e, f = (ctypes.cast(ctypes.addressof(buf) + 64 * j, ctypes.c_void_p) for j in range(6))
    inf, nan = float("inf"), float("nan")
    ok = (a, b, c, 2, 8, None)                                        # (x, w, out, N, S)
    bad = [ok[:i] + (None,) + ok[i + 1:] for i in range(3)]
    bad += [(a, b, a, 2, 8, None), (a, b, c, 0, 8, None), (a, b, c, 65536, 8, None), (a, b, c, 2, 1, None), (a, b, c, 2, 32769, None)]
    for args in bad:
        assert L.ud_flow_warp(*args) == -1000, args
    ok = (a, b, c, d, 2, 8, 1, 0.05, 1e-8, None)                      # (g, x, w, gw, N, S, sign, tau, tv_eps)
    bad = [ok[:i] + (None,) + ok[i + 1:] for i in range(4)] + [(a, b, c, c) + ok[4:]]
    bad += [ok[:4] + t + (None,) for t in ((0, 8, 1, 0.05, 1e-8), (2, 1, 1, 0.05, 1e-8), (2, 8, 0, 0.05, 1e-8), (2, 8, 2, 0.05, 1e-8),
                                           (2, 8, 1, -0.05, 1e-8), (2, 8, 1, nan, 1e-8), (2, 8, 1, inf, 1e-8), (2, 8, -1, 0.05, 0.0),
                                           (2, 8, -1, 0.05, -1.0), (2, 8, -1, 0.05, nan), (2, 8, -1, 0.05, inf))]
    for args in bad:
        assert L.ud_flow_grad(*args) == -1000, args
    ok = (a, b, c, d, 3, 4, 1, None)                                  # (f, ist, fst, history, steps, N, maximise)
    bad = [ok[:i] + (None,) + ok[i + 1:] for i in range(4)]
    bad += [ok[:4] + t + (None,) for t in ((0, 4, 1), (-1, 4, 1), (3, 0, 1), (3, -2, 0), (65535, 65536, 1))]
    for args in bad:
        assert L.ud_flow_control(*args) == -1000, args
    ok = (a, b, c, d, e, f, 2, 8, 0.25, 2.0, 0, None)                 # (w, w_best, gw, keep, x, x_adv, N, S, step, bound, closing)
    bad = [ok[:i] + (None,) + ok[i + 1:] for i in range(6)]
    bad += [(a, a) + ok[2:], (a, b, a) + ok[3:], (a, b, b) + ok[3:], ok[:5] + (e,) + ok[6:]]
    bad += [ok[:6] + t + (None,) for t in ((0, 8, 0.25, 2.0, 0), (2, 1, 0.25, 2.0, 0), (2, 8, nan, 2.0, 0), (2, 8, 0.25, -1.0, 0),
                                           (2, 8, 0.25, nan, 1), (65536, 8, 0.25, 2.0, 1))]
    bad += [args[:2] + (None,) + args[3:10] + (1, None) for args in bad[:2] + bad[3:6]]      # closing: gw may be NULL, the rest not
    for args in bad:
        assert L.ud_flow_update(*args) == -1000, args


# ---- the cache's key ----------------------------------------------------------------------------------------------------------------------
def test_cache_key(monkeypatch):
    made = []

    class Stub:
        def __init__(self, model, *args):
            made.append(args)

    monkeypatch.setattr(FL, "FlowRunner", Stub)
    m = _model()
    r = FL.flow_runner(m, 4, 128)
    assert FL.flow_runner(m, 4, 128, max_flow=2.0, steps=20) is r and m.flow_runner(4, 128, tau=0.05) is r
    assert FL.flow_runner(m, 4, 128, 2.0, 20, None, 0.05, 1e-8, False) is r and len(made) == 1
    others = [FL.flow_runner(m, 4, 128, **kw) for kw in ({"max_flow": 1.0}, {"tau": 0.0}, {"targeted": True}, {"steps": 3})]
    assert len({id(o) for o in others + [r]}) == 5 and len(made) == 5
    assert made[1][2] == 1.0 and made[2][5] == 0.0 and made[3][7] is True and made[4][3] == 3
    assert FL.flow_key(4, 128) == (4, 128, 2.0, 20, None, 0.05, 1e-8, False, "cross_entropy")
    assert FL.flow_key(4, 128, precision="fp16") == FL.flow_key(4, 128) + ("fp16", 1024.0)
    from unidefense_amd.infer import _MAX_RUNNERS
    assert len(m.__dict__["_ud_flow_runners"]) <= _MAX_RUNNERS
    assert not any(k.startswith("_ud_") and k != "_ud_flow_runners" for k in m.__dict__)          # a dictionary of its own


# ---- the stage against stubs ----------------------------------------------------------------------------------------------------------------
from tests.test_universal_cpu import DEV, Batches, expected, p0, same, logits      # noqa: E402


class StubFlow:
    """x_adv: channel 0 lowered by 0.5 on the real half (label 0), raised on the fake half; the flow's sizes grow per call"""

    def __init__(self, net, kwargs):
        self.net, self.calls = net, 0
        self.args = dict({"method": "flow", "max_flow": 2.0, "steps": 20}, **kwargs)

    def __call__(self, x, y):
        self.net.log.append("attack")
        self.calls += 1
        self.flow_linf = torch.full((x.shape[0],), 0.5 * self.calls)
        self.flow_tv = torch.arange(x.shape[0], dtype=torch.float32) + 10.0 * self.calls
        xa = x.clone()
        xa[:, 0] += torch.where(y == 0, -0.5, 0.5).view(-1, 1, 1)
        return xa


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.log, self.runner = [], None

    def forward(self, x):
        self.log.append("forward")
        return {"cls_out": logits(x)}

    def flow_runner(self, n, size, max_flow=2.0, steps=20, tau=0.05):
        self.log.append(("flow_runner", n, size))
        if self.runner is None:
            self.runner = StubFlow(self, {"max_flow": max_flow, "steps": steps, "tau": tau})
        return self.runner


def make():
    net, it = Net(), Batches()
    return evaluate.Evaluator(net, net, it, 2, 8, DEV), net, it


def test_stage_scores_clean_and_attacked(monkeypatch):
    from unidefense_amd.engine import metrics
    gathered = []
    real = metrics.gather_scores
    monkeypatch.setattr(metrics, "gather_scores", lambda s, lb: gathered.append(s) or real(s, lb))
    ev, net, it = make()
    given = {"max_flow": 1.0, "steps": 3}
    got = ev.test_flow(2, given)
    assert given == {"max_flow": 1.0, "steps": 3} and it.steps == [1, 2]
    # per batch: the runner first, the clean score, the attack, its score
    assert net.log == [("flow_runner", 4, 8), "forward", "attack", "forward"] * 2
    x, y = Batches.of([1, 2])
    xa = x.clone()
    xa[:, 0] += torch.where(y == 0, -0.5, 0.5).view(-1, 1, 1)
    want = {"clean": p0(x), "adv": p0(xa)}
    assert set(got) == {"clean", "adv", "attack"}
    for name in want:
        same(got[name], expected(want[name], y))
    assert len(gathered) == 4 and torch.equal(gathered[2], want["clean"]) and torch.equal(gathered[3], want["adv"])
    a = got["attack"]
    assert set(a) == {"method", "max_flow", "steps", "tau", "flow_linf_mean", "flow_linf_max", "flow_tv_mean", "flow_tv_max", "fooled"}
    assert (a["method"], a["max_flow"], a["steps"], a["tau"]) == ("flow", 1.0, 3, 0.05)
    assert a["flow_linf_mean"] == 0.75 and a["flow_linf_max"] == 1.0 and a["flow_tv_max"] == 23.0 and a["flow_tv_mean"] == 16.5
    right = (want["clean"] < 0.5).long() == y
    flipped = ((want["adv"] < 0.5).long() != y) & right
    assert type(a["fooled"]) is float and a["fooled"] == float(flipped.sum()) / float(right.sum()) and 0.0 <= a["fooled"] <= 1.0
    assert int(right.sum()) > 0 and a["fooled"] > 0


def test_stage_refuses_a_bad_dict():
    ev, net, it = make()
    with pytest.raises(ValueError, match="^flow takes FlowRunner's keyword arguments: .*max_flo"):
        ev.test_flow(1, {"max_flo": 1.0})
    assert "forward" not in net.log and net.runner is None
    ev = evaluate.Evaluator(_model(), _model(), it, 2, 8, DEV)      # the real accessor: its refusals pass through as they are
    with pytest.raises(ValueError, match="max_flow must be a finite number >= 0"):
        ev.test_flow(1, {"max_flow": -1.0})
    with pytest.raises(ValueError, match="flow takes FlowRunner's keyword arguments"):
        ev.test_flow(1, {"eps": 0.1})
    assert list(evaluate.ROBUST) == ["pgd", "apgd", "square", "apgd+square", "fmn", "sparse_fmn"]      # the stage is no ROBUST method
    from unidefense_amd.engine.train_engine import TrainEngine
    assert callable(TrainEngine.test_flow)
