"""CPU: the attribution's host side (unidefense_amd/attrib.py, engine/evaluate.py: test_attribution): the quadrature tables, the
rank rule on hand-made maps, the trapezoid, every refusal without a device, the runner caches, the six entry points' argument
tests, the header's rows and modes, and the stage's rules against stubs."""
import ctypes
import inspect
import math
import re

import numpy as np
import pytest
import torch

from unidefense_amd import attrib as A
from unidefense_amd.engine import evaluate, metrics

ONES = 0xFFFFFFFFFFFFFFFF


def _model():
    from unidefense_amd.model import load_model
    return load_model("UDR18")(num_classes=2).eval()


# ---- the quadrature -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", A.RULES)
def test_schedule_weights_sum_to_one_and_nodes_are_symmetric(rule):
    for m in (1, 2, 3, 4, 5, 8, 16, 32, 33, 64):
        a, w = A.attribution_schedule(m, rule)
        assert a.dtype == w.dtype == np.float64 and a.shape == w.shape == (m,)
        assert abs(math.fsum(w) - 1.0) <= 1e-15, m
        assert np.abs(a + a[::-1] - 1.0).max() <= 1e-15, m          # symmetric about 1/2
        assert np.all(np.diff(a) > 0) and 0.0 < a[0] and a[-1] < 1.0 and np.all(w > 0)


def test_gauss_legendre_is_exact_to_degree_2m_minus_1_and_no_further():
    for m in (1, 2, 3, 4, 8):
        a, w = A.attribution_schedule(m, "gauss_legendre")
        assert abs(math.fsum(w * a ** (2 * m - 1)) - 1.0 / (2 * m)) <= 1e-14, m
        assert abs(math.fsum(w * a ** (2 * m)) - 1.0 / (2 * m + 1)) > 1e-10, m
    a, w = A.attribution_schedule(2, "gauss_legendre")
    assert np.allclose(a, [0.5 - 0.5 / math.sqrt(3), 0.5 + 0.5 / math.sqrt(3)], rtol=0, atol=1e-16) and w.tolist() == [0.5, 0.5]


def test_midpoint_nodes_and_schedule_refusals():
    for m in (1, 2, 7):
        a, w = A.attribution_schedule(m, "midpoint")
        assert a.tolist() == [(i + 0.5) / m for i in range(m)] and w.tolist() == [1.0 / m] * m
    a, w = A.attribution_schedule(2, "midpoint")
    assert abs(math.fsum(w * a ** 2) - 1 / 3) == pytest.approx(1 / 48)          # h^2 / 24 f'' with h = 1/2, f'' = 2
    with pytest.raises(ValueError, match="rule must be one of"):
        A.attribution_schedule(4, "simpson")
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="steps must be an integer >= 1"):
            A.attribution_schedule(bad)


def test_known_integrand_bar_holds_for_the_restatement_and_rejects_the_midpoint_rule():
    """tests/test_v_attrib_gpu.py's case 3 on the host: in float64 with the fp32-rounded nodes, two Gauss-Legendre nodes stay
    inside a quarter of the derived bar and two midpoint nodes exceed ten times it."""
    from tests import attrib_case as AC
    x, b, _, _ = AC.inputs()
    want = AC.exact(x, b)
    total, bar = AC.restated(x, b, "gauss_legendre")
    err = np.abs(total - want)
    print("  gauss_legendre |total - (F(x) - F(b))| / bar:", (err / bar).tolist())
    assert np.all(err <= 0.25 * bar)
    total, bar = AC.restated(x, b, "midpoint")
    assert np.all(np.abs(total - want) > 10 * bar)


# ---- the rank rule ------------------------------------------------------------------------------------------------------------------
def _top(heat, kcount):
    """per j the sorted pixel indices with key >= threshold"""
    keys, thr = A.ref_rank_keys(heat), A.ref_rank_select(heat, kcount)
    assert thr.dtype == np.uint64 and thr.shape == (len(kcount), keys.shape[0])
    return [[np.flatnonzero(keys[n] >= thr[j, n]).tolist() for n in range(keys.shape[0])] for j in range(len(kcount))]


def test_rank_select_on_hand_made_maps():
    nan = float("nan")
    # all equal: the lowest indices win
    top = _top(np.full((1, 6), 0.25, dtype=np.float32), [0, 1, 3, 6])
    assert [t[0] for t in top] == [[], [0], [0, 1, 2], [0, 1, 2, 3, 4, 5]]
    # a NaN ranks last, also behind -inf; negatives order by value
    h = np.array([[-1.0, nan, 3.0, -float("inf"), -2.5, 0.5]], dtype=np.float32)
    top = _top(h, [1, 2, 3, 4, 5, 6])
    assert [t[0] for t in top] == [[2], [2, 5], [0, 2, 5], [0, 2, 4, 5], [0, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5]]
    # the two zeros tie: the lower index first, whichever sign it has
    h = np.array([[-0.0, 0.0, -1.0, 0.0, -0.0, 1.0]], dtype=np.float32)
    top = _top(h, [1, 2, 3, 4, 5])
    assert [t[0] for t in top] == [[5], [0, 5], [0, 1, 5], [0, 1, 3, 5], [0, 1, 3, 4, 5]]
    # kcount 0: all ones, nobody is above it; kcount HW: everybody; more than one sample, each with its own threshold
    h = np.array([[1.0, 2.0, 3.0, 4.0], [4.0, 3.0, 2.0, 1.0], [nan, nan, nan, nan]], dtype=np.float32)
    thr = A.ref_rank_select(h, [0, 2, 4])
    assert thr[0].tolist() == [ONES] * 3
    keys = A.ref_rank_keys(h)
    assert keys.max() < ONES and len(set(keys[2].tolist())) == 4
    assert [np.flatnonzero(keys[n] >= thr[1, n]).tolist() for n in range(3)] == [[2, 3], [0, 1], [0, 1]]
    assert all(int((keys[n] >= thr[2, n]).sum()) == 4 for n in range(3))
    # exactly kcount keys are >= the threshold, on a map with massive ties
    g = np.random.default_rng(5)
    h = g.integers(0, 4, size=(2, 1089)).astype(np.float32)
    kc = [0, 1, 363, 1088, 1089]
    thr = A.ref_rank_select(h, kc)
    keys = A.ref_rank_keys(h)
    assert [[int((keys[n] >= thr[j, n]).sum()) for n in range(2)] for j in range(5)] == [[k, k] for k in kc]
    # the integer order of the keys IS the order of the stable sort
    order = np.argsort(-h[0].astype(np.float64), kind="stable")
    assert np.array_equal(np.argsort(keys[0])[::-1], order)


def test_rank_keys_layout():
    h = np.array([[1.0, -1.0, 0.0, float("nan"), float("inf"), -float("inf")]], dtype=np.float32)
    k = A.ref_rank_keys(h)[0].tolist()
    assert [v >> 32 for v in k] == [0xBF800000, 0x407FFFFF, 0x80000000, 0, 0xFF800000, 0x007FFFFF]
    assert [v & 0xFFFFFFFF for v in k] == [0xFFFFFFFF - p for p in range(6)]


def test_ref_mask_on_a_hand_made_image():
    x = np.arange(24, dtype=np.float32).reshape(2, 3, 2, 2) + 1
    b = -np.ones_like(x)
    heat = np.array([[[0.0, 2.0], [1.0, 2.0]], [[5.0, 5.0], [5.0, 5.0]]], dtype=np.float32)
    thr = A.ref_rank_select(heat, [0, 1, 2, 4])
    d = A.ref_attr_mask(x, b, heat, thr, [2, 1], "deletion")
    assert d[0, :, 0, 1].tolist() == [-1] * 3 and d[0, :, 1, 1].tolist() == [-1] * 3 and np.array_equal(d[0, :, :, 0], x[0, :, :, 0])
    assert d[1, :, 0, 0].tolist() == [-1] * 3 and int((d[1] != x[1]).sum()) == 3
    i = A.ref_attr_mask(x, b, heat, thr, [2, 1], "insertion")
    assert np.array_equal(np.where(d == x, b, x), i)                    # the complement, pixel by pixel
    assert np.array_equal(A.ref_attr_mask(x, b, heat, thr, [3, 3], "deletion"), b)
    assert np.array_equal(A.ref_attr_mask(x, b, heat, thr, [3, 0], "insertion"), np.stack([x[0], b[1]]))
    with pytest.raises(ValueError, match="mode must be one of"):
        A.ref_attr_mask(x, b, heat, thr, [0, 0], "blur")


def test_ref_point_accumulate_finish_rules():
    x = np.array([[1.0, np.nan, 0.3], [0.5, 0.25, -0.0]], dtype=np.float32)
    b = np.array([[-1e-8, 0.0, -1.0], [-1.0, -1.0, -1.0]], dtype=np.float32)
    alpha = np.array([0.0, 1.0, 0.5], dtype=np.float32)
    old = np.full_like(x, 7.0)
    got = A.ref_attr_point(x, b, old, [1, 3], alpha, 3)
    assert np.array_equal(got[0], x[0], equal_nan=True) and got[1].tolist() == [7.0] * 3        # a == 1: x; k outside: untouched
    got = A.ref_attr_point(x, b, old, [0, 2], alpha, 6)
    assert np.array_equal(got[0], b[0]) and got[1].tolist() == [-0.25, -0.375, -0.5]              # a == 0: b, also under a NaN x
    got = A.ref_attr_point(x, b, old, [5, -1], alpha, 6)                                          # node 5 % 3
    assert np.isnan(got[0, 1]) and got[0, 2] == np.float32(-1.0) + np.float32(0.5) * (np.float32(0.3) - np.float32(-1.0))
    acc = A.ref_attr_accumulate(np.array([[1.0, 2.0]], dtype=np.float32), np.array([[0.5, 0.5]]), [1], [0.25, 0.125], 2)
    assert acc.dtype == np.float64 and acc.tolist() == [[0.625, 0.75]]
    xi = np.arange(12, dtype=np.float32).reshape(1, 3, 2, 2)
    ac = np.full((1, 3, 2, 2), 0.5)
    ac[0, 1] = -0.5
    attr, heat, v = A.ref_attr_finish(xi, np.ones_like(xi), ac, "ig", "sum", 0.5)
    assert attr.dtype == heat.dtype == np.float32 and v.dtype == np.float64
    assert np.array_equal(v, (xi.astype(np.float64) - 1) * ac * 0.5) and np.array_equal(heat[0], (v[0, 0] + v[0, 1] + v[0, 2]))
    _, habs, _ = A.ref_attr_finish(xi, np.ones_like(xi), ac, "ig", "abs", 0.5)
    assert np.array_equal(habs[0], np.abs(v[0]).sum(0).astype(np.float32))
    g, _, vg = A.ref_attr_finish(xi, np.ones_like(xi), ac, "grad", "sum", 2.0)
    assert np.array_equal(vg, ac * 2.0) and np.array_equal(g, (ac * 2).astype(np.float32))


# ---- the curve's host side ----------------------------------------------------------------------------------------------------------
def test_trapezoid_auc_and_counts():
    curve = np.array([[1.0, 0.0], [0.5, 0.0], [0.25, 1.0], [0.0, 1.0]], dtype=np.float32)
    auc = A.trapezoid_auc(curve, [0.0, 0.25, 0.5, 1.0])
    assert auc.dtype == np.float64 and auc.tolist() == [0.25 * 0.75 + 0.25 * 0.375 + 0.5 * 0.125, 0.25 * 0.0 + 0.25 * 0.5 + 0.5 * 1.0]
    assert A.trapezoid_auc(np.ones((3, 1)), [0.0, 0.5, 1.0]).tolist() == [1.0]
    assert A.trapezoid_auc(curve[:2], [0.5, 0.5]).tolist() == [0.0, 0.0]                   # a repeated fraction has no width
    assert A.deletion_counts(A.DEFAULT_FRACTIONS, 128) == [0, 328, 819, 1638, 3277, 5734, 8192, 12288, 16384]
    assert A.deletion_counts((0, 0.5, 1), 1) == [0, 1, 1] and A.deletion_counts((0, 0.5, 1), 3) == [0, 5, 9]
    assert A.deletion_counts((1 / 3, 2 / 3), 33) == [363, 726]


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
BAD = [({"method": "lime"}, "method must be one of ('ig', 'smoothgrad')"), ({"steps": 0}, "steps must be an integer >= 1"),
       ({"steps": 2.5}, "steps must be an integer >= 1"), ({"rule": "simpson"}, "rule must be one of ('gauss_legendre', 'midpoint')"),
       ({"baseline": "blur"}, "baseline must be one of ('black', 'grey', 'given')"), ({"baseline": None}, "baseline must be one of"),
       ({"samples": 0}, "samples must be an integer >= 1"), ({"steps": 1 << 16, "samples": 1 << 15}, "steps * samples must stay below 2^31"),
       ({"sigma": -0.1}, "sigma must be finite and >= 0"), ({"sigma": float("inf")}, "sigma must be finite and >= 0"),
       ({"sigma": float("nan")}, "sigma must be finite and >= 0"), ({"sigma": None}, "sigma must be finite and >= 0"),
       ({"score": "loss"}, "score must be one of ('margin', 'logit') or a callable"), ({"score": None}, "score must be one of"),
       ({"reduce": "max"}, "reduce must be one of ('sum', 'abs')"), ({"seed": 1.5}, "seed must be an integer"),
       ({"precision": "bf16"}, "precision"), ({"precision": "fp16"}, "fp16"), ({"grad_scale": 3.0}, "grad_scale"),
       ({"precision": "fp32", "grad_scale": 1024.0}, "grad_scale")]


@pytest.mark.parametrize("kw,text", BAD)
def test_attribution_refusals_need_no_device(kw, text):
    m = _model()
    for make in (lambda: A.AttributionRunner(m, 2, 64, **kw), lambda: A.attribution_runner(m, 2, 64, **kw),
                 lambda: m.attribution_runner(2, 64, **kw)):
        with pytest.raises(ValueError, match=re.escape(text)):
            make()
    assert not m.__dict__.get("_ud_attribution_runners")


BAD_CURVE = [({"fractions": ()}, "fractions must hold at least two"), ({"fractions": (0.5,)}, "fractions must hold at least two"),
             ({"fractions": (0, 1.5)}, "fractions must hold"), ({"fractions": (0, -0.1)}, "fractions must hold"),
             ({"fractions": (0.5, 0.2)}, "non-decreasing"), ({"fractions": (0, float("nan"))}, "fractions must hold"),
             ({"fractions": None}, "fractions must hold"), ({"mode": "blur"}, "mode must be one of ('deletion', 'insertion')"),
             ({"baseline": "white"}, "baseline must be one of"), ({"score": "margin"}, "score must be one of ('prob',) or a callable"),
             ({"precision": "bf16"}, "precision"), ({"precision": "fp16"}, "fp16")]


@pytest.mark.parametrize("kw,text", BAD_CURVE)
def test_deletion_refusals_need_no_device(kw, text):
    m = _model()
    for make in (lambda: A.DeletionRunner(m, 2, 64, **kw), lambda: A.deletion_runner(m, 2, 64, **kw),
                 lambda: m.deletion_runner(2, 64, **kw)):
        with pytest.raises(ValueError, match=re.escape(text)):
            make()
    assert not m.__dict__.get("_ud_deletion_runners")


def test_host_side_refusals_defaults_and_accessors():
    from unidefense_amd.model import load_model
    m = load_model("UDR18")(num_classes=2)
    for cls in (A.AttributionRunner, A.DeletionRunner):
        with pytest.raises(ValueError, match="eval"):
            cls(m.train(), 2, 64)
        with pytest.raises(ValueError, match="cuda"):            # only the device is missing
            cls(m.eval(), 2, 64)
        with pytest.raises(ValueError, match="takes a UDEB4"):
            cls(torch.nn.Linear(2, 2), 2, 64)
    with pytest.raises(ValueError, match="cuda"):
        A.AttributionRunner(m.eval(), 2, 64, "smoothgrad", 4, "midpoint", "given", 3, 0.1, lambda out, y, xp: y, "abs", 1 << 40)
    for name in ("UDEB4", "UDR18", "UDR50"):
        assert callable(getattr(load_model(name), "attribution_runner")) and callable(getattr(load_model(name), "deletion_runner"))
    a = A._attribution_arguments(4, 128)
    assert list(a) == ["batch", "size", "method", "steps", "rule", "baseline", "samples", "sigma", "score", "reduce", "seed",
                       "precision", "grad_scale"]
    assert tuple(a.values())[2:] == ("ig", 32, "gauss_legendre", "black", 1, 0.0, "margin", "sum", 0, "fp32", None)
    d = A._deletion_arguments(4, 128)
    assert list(d) == ["batch", "size", "fractions", "mode", "baseline", "score", "precision"]
    assert tuple(d.values())[2:] == ((0, .02, .05, .1, .2, .35, .5, .75, 1), "deletion", "black", "prob", "fp32")
    assert A.DeletionRunner._backward is False and A.AttributionRunner._backward is True
    assert A.BASELINE_VALUE == {"black": -1.0, "grey": 0.0}


def test_score_helpers():
    out = {"cls_out": torch.tensor([[2.0, -1.0], [0.5, 0.25]])}
    y = torch.tensor([1, 0])
    assert A.logit_each(out, y).tolist() == [-1.0, 0.5]
    assert torch.equal(A.prob_each(out, y), torch.softmax(out["cls_out"], 1)[torch.arange(2), y])
    one = {"cls_out": torch.tensor([[2.0], [-3.0]])}
    assert A.logit_each(one, y).tolist() == [2.0, 3.0]
    assert torch.equal(A.prob_each(one, y), torch.sigmoid(torch.tensor([2.0, 3.0])))


# ---- the caches ---------------------------------------------------------------------------------------------------------------------
def test_cache_keys(monkeypatch):
    made = []

    class Stub:
        def __init__(self, model, *args):
            made.append(args)

    monkeypatch.setattr(A, "AttributionRunner", Stub)
    monkeypatch.setattr(A, "DeletionRunner", Stub)
    m = _model()

    def hook(out, y, xp):
        return None

    def other(out, y, xp):
        return None

    from unidefense_amd.infer import _MAX_RUNNERS
    r = A.attribution_runner(m, 4, 128)
    assert A.attribution_runner(m, 4, 128) is r and m.attribution_runner(4, 128, method="ig", steps=32, rule="gauss_legendre") is r
    assert A.attribution_runner(m, 4, 128, "ig", 32, "gauss_legendre", "black", 1, 0.0, "margin", "sum", 0) is r and len(made) == 1
    others = [A.attribution_runner(m, 4, 128, **kw) for kw in ({"steps": 8}, {"rule": "midpoint"}, {"score": hook})]
    assert len({id(o) for o in others + [r]}) == 4 and len(made) == 4
    assert A.attribution_runner(m, 4, 128, score=hook) is others[2]                      # a callable is keyed by identity
    assert A.attribution_runner(m, 4, 128, score=other) is not others[2]
    # constructor arguments after the model: (batch, size, method, steps, rule, baseline, samples, sigma, score, ...)
    assert made[-1][8] is other and made[3][8] is hook and made[1][3] == 8 and made[2][4] == "midpoint"
    assert len(made) == 5 and len(m.__dict__["_ud_attribution_runners"]) == _MAX_RUNNERS < len(made)
    assert r not in m.__dict__["_ud_attribution_runners"].values()                       # the oldest went first
    assert not any(k.startswith("_ud_") and k != "_ud_attribution_runners" for k in m.__dict__)      # a dictionary of its own
    before = dict(m.__dict__["_ud_attribution_runners"])
    made.clear()
    d = A.deletion_runner(m, 4, 128)
    assert A.deletion_runner(m, 4, 128, fractions=list(A.DEFAULT_FRACTIONS)) is d and m.deletion_runner(4, 128, mode="deletion") is d
    i = m.deletion_runner(4, 128, mode="insertion")
    assert i is not d and m.deletion_runner(4, 128, score=hook) is m.deletion_runner(4, 128, score=hook) and len(made) == 3
    assert m.deletion_runner(4, 128, fractions=(0, 1)) is not d and m.deletion_runner(4, 128, baseline="grey") is not d
    assert len(made) == 5 and len(m.__dict__["_ud_deletion_runners"]) == _MAX_RUNNERS
    assert d not in m.__dict__["_ud_deletion_runners"].values()
    assert m.__dict__["_ud_attribution_runners"] == before                               # each kind in its own dictionary


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
NAMES = {"ud_attr_point": ["x", "b", "xp", "k", "alpha", "steps", "iters", "N", "per", "stream"],
         "ud_attr_accumulate": ["g", "acc", "k", "w", "steps", "iters", "N", "per", "stream"],
         "ud_attr_control": ["f", "ist", "path", "N", "iters", "stream"],
         "ud_attr_finish": ["x", "b", "acc", "attr", "heat", "total", "ws", "ws_bytes", "mode", "reduce", "scale", "N", "S", "stream"],
         "ud_attr_rank_select": ["heat", "kcount", "thr", "N", "HW", "K", "stream"],
         "ud_attr_mask": ["x", "b", "heat", "thr", "ist", "xq", "mode", "N", "S", "K", "stream"]}


def test_entry_points_are_declared_exported_and_refuse_bad_arguments():
    from tests.test_abi_cpu import header
    from unidefense_amd import kernels as K
    from unidefense_amd import lib
    h = header()
    L = ctypes.CDLL(lib.LIB_PATH)
    for n, names in NAMES.items():
        assert n in h.protos and n in lib.EXPORTED and hasattr(L, n), n
        assert h.protos[n][0] is ctypes.c_int and [name for _, name in h.protos[n][1]] == names, n
        fn = getattr(L, n)
        fn.restype, fn.argtypes = ctypes.c_int, [t for t, _ in h.protos[n][1]]
    assert h.protos["ud_attr_finish_ws_bytes"][0] is ctypes.c_int
    L.ud_attr_finish_ws_bytes.restype, L.ud_attr_finish_ws_bytes.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_long]
    for n in ("attr_point", "attr_accumulate", "attr_control", "attr_finish", "attr_finish_ws_bytes", "attr_rank_select", "attr_mask"):
        assert callable(getattr(K, n)), n
    rows = {k[len("UD_ATTR_I_"):].lower(): v for k, v in h.consts.items() if k.startswith("UD_ATTR_I_")}
    assert K.ATTR_I == rows == {"k": 0}
    assert K.ATTR_MODE == {"ig": h.consts["UD_ATTR_IG"], "grad": h.consts["UD_ATTR_GRAD"]} == {"ig": 0, "grad": 1}
    assert K.ATTR_REDUCE == {"sum": h.consts["UD_ATTR_SUM"], "abs": h.consts["UD_ATTR_ABS"]} == {"sum": 0, "abs": 1}
    assert tuple(K.ATTR_REDUCE) == A.REDUCES
    assert K.ATTR_MASK == {"deletion": h.consts["UD_ATTR_DELETE"], "insertion": h.consts["UD_ATTR_INSERT"]} == {"deletion": 0, "insertion": 1}
    assert tuple(K.ATTR_MASK) == A.MODES
    # the workspace: one double per workgroup of 1024 pixels, per sample; a function of per alone per sample
    ws = L.ud_attr_finish_ws_bytes
    assert ws(1, 3) == 8 and ws(5, 3) == 40 and ws(1, 3 * 1024) == 8 and ws(1, 3 * 1025) == 16 and ws(2, 3 * 256 * 256) == 2 * 64 * 8
    assert [ws(*a) for a in ((0, 3), (65536, 3), (1, 0), (1, 4), (1, -3), (40000, 3 << 23))] == [-1000] * 6
    assert ws(32767, 3 << 23) == 32767 * 8192 * 8                     # 8192 parts per sample: the largest workspace an int holds

    buf = (ctypes.c_double * 128)()
    p = [ctypes.cast(ctypes.addressof(buf) + 128 * j, ctypes.c_void_p) for j in range(7)]
    nan = float("nan")

    def refused(fn, ok, pointers, scalars):
        """every pointer of `ok` as NULL, and `ok` with its trailing scalars replaced by each of `scalars`"""
        bad = [ok[:i] + (None,) + ok[i + 1:] for i in pointers]
        bad += [ok[:len(ok) - len(s) - 1] + tuple(s) + (None,) for s in scalars]
        for args in bad:
            assert fn(*args) == -1000, (fn.__name__, args)

    # (x, b, xp, k, alpha, steps, iters, N, per)
    sizes = [(0, 4, 2, 12), (2, 0, 2, 12), (2, 4, 0, 12), (2, 4, -1, 12), (2, 4, 65536, 12), (2, 4, 2, 0), (2, 4, 2, -12), (-2, 4, 2, 12),
             (2, -4, 2, 12), (2, 1 << 30, 2, 12), (2, 65536, 65535, 12), (2, 4, 2, 1 << 41)]
    refused(L.ud_attr_point, (p[0], p[1], p[2], p[3], p[4], 2, 4, 2, 12, None), range(5), sizes)
    # (g, acc, k, w, steps, iters, N, per)
    refused(L.ud_attr_accumulate, (p[0], p[1], p[2], p[3], 2, 4, 2, 12, None), range(4), sizes)
    # (f, ist, path, N, iters)
    refused(L.ud_attr_control, (p[0], p[1], p[2], 2, 4, None), range(3),
            [(0, 4), (-1, 4), (65536, 4), (2, 0), (2, -1), (2, 1 << 30), (65535, 65536)])
    # (x, b, acc, attr, heat, total, ws, ws_bytes, mode, reduce, scale, N, S)
    refused(L.ud_attr_finish, (p[0], p[1], p[2], p[3], p[4], p[5], p[6], 1024, 0, 0, 1.0, 2, 2, None), range(7),
            [(8, 0, 0, 1.0, 2, 2), (0, 0, 0, 1.0, 2, 2), (-8, 0, 0, 1.0, 2, 2), (1024, 2, 0, 1.0, 2, 2), (1024, -1, 0, 1.0, 2, 2),
             (1024, 0, 2, 1.0, 2, 2), (1024, 0, -1, 1.0, 2, 2), (1024, 0, 0, nan, 2, 2), (1024, 0, 0, 1.0, 0, 2),
             (1024, 0, 0, 1.0, 65536, 2), (1024, 0, 0, 1.0, 2, 0), (1024, 0, 0, 1.0, 2, -2), (1024, 0, 0, 1.0, 2, 32769)])
    # (heat, kcount, thr, N, HW, K)
    refused(L.ud_attr_rank_select, (p[0], p[1], p[2], 2, 4, 3, None), range(3),
            [(0, 4, 3), (-1, 4, 3), (65536, 4, 3), (2, 0, 3), (2, -4, 3), (2, (1 << 30) + 1, 3), (2, 4, 0), (2, 4, -3), (2, 4, 1 << 30)])
    # (x, b, heat, thr, ist, xq, mode, N, S, K)
    refused(L.ud_attr_mask, (p[0], p[1], p[2], p[3], p[4], p[5], 0, 2, 2, 3, None), range(6),
            [(2, 2, 2, 3), (-1, 2, 2, 3), (0, 0, 2, 3), (0, 65536, 2, 3), (0, 2, 0, 3), (0, 2, 32769, 3), (0, 2, 2, 0), (0, 2, 2, -1),
             (1, 2, 2, 1 << 30)])


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from unidefense_amd import kernels as K
    x, heat = torch.zeros(2, 3, 4, 4), torch.zeros(2, 4, 4)
    k, ist = torch.zeros(2, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32)
    acc, total = torch.zeros(2, 3, 4, 4, dtype=torch.float64), torch.zeros(2, dtype=torch.float64)
    thr = torch.zeros(3, 2, dtype=torch.int64)
    for call in (lambda: K.attr_point(x, x.clone(), x.clone(), k, torch.ones(2), 2),
                 lambda: K.attr_accumulate(x, acc, k, torch.ones(2, dtype=torch.float64), 2),
                 lambda: K.attr_control(torch.zeros(2), ist, torch.zeros(3, 2)),
                 lambda: K.attr_finish(x, x.clone(), acc, x.clone(), heat, total),
                 lambda: K.attr_rank_select(heat, torch.zeros(3, dtype=torch.int32), thr),
                 lambda: K.attr_mask(x, x.clone(), heat, thr, ist, x.clone())):
        with pytest.raises(ValueError, match="CUDA"):
            call()


# ---- the stage against stubs --------------------------------------------------------------------------------------------------------
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


class StubAttribution:
    """heat = the channel sum of x; gap and the scores hand-made; buffers that the next call overwrites"""

    def __init__(self, net, kwargs):
        self.net = net
        self.args = dict({"method": "ig", "steps": 32, "rule": "gauss_legendre", "baseline": "black", "seed": 3}, **kwargs)
        self.heat, self.gap = torch.zeros(4, 8, 8), torch.zeros(4, dtype=torch.float64)
        self.f_x, self.f_b = torch.zeros(4), torch.zeros(4)

    def __call__(self, x, y, ids=None, baseline=None):
        self.net.log.append(("attribution", float(x.sum()), ids.tolist()))
        self.heat.copy_(x.sum(1))
        self.gap.copy_(torch.tensor([0.5, -0.25, 0.0, 1.0], dtype=torch.float64) * (1 + ids[0]))
        self.f_x.copy_(torch.tensor([2.0, 1.0, 0.0, -3.0]))
        self.f_b.copy_(torch.tensor([1.0, 2.0, 0.0, 1.0]))
        return x


class StubCurve:
    """auc = the heat map's mean (deletion) or maximum (insertion), in a buffer that the next call overwrites"""

    def __init__(self, net, mode, kwargs):
        self.net, self.mode, self.args = net, mode, dict({"fractions": A.DEFAULT_FRACTIONS, "mode": mode}, **kwargs)
        self.auc = torch.zeros(4, dtype=torch.float64)

    def __call__(self, x, y, heat, baseline=None):
        self.net.log.append((self.mode, float(heat.double().sum())))
        self.auc.copy_(heat.double().flatten(1).mean(1) if self.mode == "deletion" else heat.double().flatten(1).amax(1))
        return self.auc


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.log, self.runner, self.curves = [], None, {}

    def forward(self, x):
        self.log.append("forward")
        return {"cls_out": logits(x)}

    def attribution_runner(self, n, size, method="ig", steps=32, baseline="black", seed=3):
        self.log.append(("attribution_runner", n, size))
        if steps < 1:
            raise ValueError("steps must be an integer >= 1")
        if self.runner is None:
            self.runner = StubAttribution(self, {"method": method, "steps": steps, "baseline": baseline, "seed": seed})
        return self.runner

    def deletion_runner(self, n, size, fractions=A.DEFAULT_FRACTIONS, mode="deletion", baseline="black", precision="fp32"):
        self.log.append(("deletion_runner", n, size, mode, baseline, precision))
        A._refuse_fractions(fractions)
        return self.curves.setdefault(mode, StubCurve(self, mode, {"fractions": tuple(fractions)}))


def host_noise(x, out, ids, k, draw0, mode, scale, seed):
    """kernels.smooth_noise's host stand-in: the restatement, which draws no torch generator"""
    from unidefense_amd.smooth import ref_smooth_noise
    assert k is None and draw0 == 0 and mode == "uniform" and scale == 1.0 and not x.any()
    return out.copy_(torch.from_numpy(ref_smooth_noise(x, ids, 0, mode, scale, seed)))


def make():
    net, it = Net(), Batches()
    return evaluate.Evaluator(net, net, it, 2, 8, DEV), net, it


def test_stage_order_columns_and_no_generator(monkeypatch, capsys):
    from unidefense_amd.smooth import ref_smooth_noise
    gathered = []
    real = metrics.gather_scores
    monkeypatch.setattr(metrics, "gather_scores", lambda s, lb: gathered.append(s) or real(s, lb))
    ev, net, it = make()
    given = {"steps": 8, "fractions": [0, 0.5, 1]}
    state = torch.get_rng_state()
    got = ev.test_attribution(2, given, noise=host_noise)
    assert torch.equal(torch.get_rng_state(), state)                             # no generator drawn
    assert given == {"steps": 8, "fractions": [0, 0.5, 1]}                       # the caller's dict is not consumed
    assert it.steps == [1, 2]
    xs = [Batches.of([s])[0] for s in (1, 2)]
    rnd = [torch.from_numpy(ref_smooth_noise(np.zeros((4, 64), dtype=np.float32), np.arange(4) + 4 * i, 0, "uniform", 1.0, 3))
           for i in range(2)]
    assert all(float(r.abs().max()) < 1 and not (r == 0).any() for r in rnd) and not torch.equal(rnd[0], rnd[1])
    want = [("attribution_runner", 4, 8), ("deletion_runner", 4, 8, "deletion", "black", "fp32"),
            ("deletion_runner", 4, 8, "insertion", "black", "fp32")]
    for i, x in enumerate(xs):        # per batch: the clean score, the map with the run's stream ids, its curves, the random map's
        want += ["forward", ("attribution", float(x.sum()), [4 * i + j for j in range(4)]),
                 ("deletion", float(x.sum(1).double().sum())), ("insertion", float(x.sum(1).double().sum())),
                 ("deletion", float(rnd[i].double().sum())), ("insertion", float(rnd[i].double().sum()))]
    assert net.log == want
    x, y = Batches.of([1, 2])
    heat, rand = x.sum(1).double().flatten(1), torch.cat(rnd).double()
    # seven gathers, in this order; every column was cloned per batch (the stubs overwrite their buffers)
    assert len(gathered) == 7
    for got_col, want_col in zip(gathered, (heat.mean(1), heat.amax(1), rand.mean(1), rand.amax(1))):
        assert torch.equal(got_col, want_col)
    gap = torch.tensor([0.5, -0.25, 0.0, 1.0, 2.5, -1.25, 0.0, 5.0], dtype=torch.float64)
    assert torch.equal(gathered[4], gap) and torch.equal(gathered[5], torch.tensor([1.0, -1.0, 0.0, -4.0] * 2, dtype=torch.float64))
    assert torch.equal(gathered[6], p0(x))
    assert set(got) == {"clean", "deletion_auc", "insertion_auc", "gap_rel", "attribution"}
    assert torch.equal(got["clean"]["scores"], p0(x)) and torch.equal(got["clean"]["labels"], y) and "AUC" in got["clean"]
    assert got["attribution"] == {"method": "ig", "steps": 8, "rule": "gauss_legendre", "baseline": "black", "seed": 3,
                                  "fractions": (0, 0.5, 1)}
    d, i = got["deletion_auc"], got["insertion_auc"]
    assert set(d) == set(i) == {"ig", "random", "per_sample"}
    assert d["ig"] == float(heat.mean(1).mean()) and d["random"] == float(rand.mean(1).mean())
    assert i["ig"] == float(heat.amax(1).mean()) and i["random"] == float(rand.amax(1).mean())
    assert torch.equal(d["per_sample"]["ig"], heat.mean(1)) and torch.equal(i["per_sample"]["random"], rand.amax(1))
    tiny = torch.finfo(torch.float64).tiny
    assert got["gap_rel"].dtype == torch.float64
    assert got["gap_rel"].tolist() == [0.5, 0.25, 0.0, 0.25, 2.5, 1.25, 0.0, 1.25] and 1.0 / tiny > 1e300      # 0 / tiny = 0: finite
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Test(attribution")]
    assert len(lines) == 1 and "8 steps" in lines[0]


def test_stage_refusals_fire_before_any_batch():
    ev, net, it = make()
    with pytest.raises(ValueError, match="^attribution takes AttributionRunner's keyword arguments and 'fractions': .*stepz"):
        ev.test_attribution(1, {"stepz": 4}, noise=host_noise)
    with pytest.raises(ValueError, match="steps must be an integer >= 1"):
        ev.test_attribution(1, {"steps": 0}, noise=host_noise)
    with pytest.raises(ValueError, match="fractions must hold"):
        ev.test_attribution(1, {"fractions": [0.5, 0.1]}, noise=host_noise)
    with pytest.raises(ValueError, match="baseline must be 'black' or 'grey'"):
        make()[0].test_attribution(1, {"baseline": "given"}, noise=host_noise)
    for batches in (0, 1.5):
        with pytest.raises(ValueError, match="batches must be an integer >= 1"):
            ev.test_attribution(batches, {}, noise=host_noise)
    assert it.steps == [] and "forward" not in net.log
    # the real accessor's refusals are ValueErrors already: they pass through, before any batch
    ev = evaluate.Evaluator(_model(), _model(), it, 2, 8, DEV)
    with pytest.raises(ValueError, match="rule must be one of"):
        ev.test_attribution(1, {"rule": "simpson"})
    with pytest.raises(ValueError, match="attribution takes AttributionRunner's keyword arguments and 'fractions'"):
        ev.test_attribution(1, {"eps": 0.1})
    assert it.steps == []


def test_engine_method_reads_the_config_default():
    from unidefense_amd.engine.train_engine import TrainEngine
    sig = inspect.signature(TrainEngine.test_attribution)
    assert list(sig.parameters) == ["self", "batches", "attribution"]
    assert sig.parameters["batches"].default == 4 and sig.parameters["attribution"].default is None
    seen = []

    class Ev:
        def test_attribution(self, batches, attribution):
            seen.append((batches, attribution))
            return "ret"

    class Engine:
        config = {"config": {"attribution": {"steps": 16}}}

        def _evaluator(self):
            return Ev()

    assert TrainEngine.test_attribution(Engine(), 2) == "ret" and TrainEngine.test_attribution(Engine(), 3, {"steps": 7}) == "ret"
    assert seen == [(2, {"steps": 16}), (3, {"steps": 7})]
