"""GPU: the warp kernel (csrc/warp.hip) against its numpy restatement (tests/test_spatial_cpu.py: ref_warp) bit for bit, the
table contract, ud_spatial_control against a Python loop, SpatialRunner's life cycle and what it leaves alone, and the engine's
test_spatial stage.

The shapes are the smallest at which the kernel can go wrong with its 32 x 32 tile: 8 (less than a tile), 20 (a side that is no
multiple of it), 44 (a full tile and a part of one) and 128 (four tiles both ways), N = 1 and 3; 256 and 380 (a last tile of 28)
once each.  Scale 0.25 makes a full tile's source box larger than the staged budget: those workgroups take the direct path."""
import copy

import numpy as np
import pytest
import torch

from oracle import param_fill
from tests import oracle_util as ou
from tests.test_corrupt_cpu import ref_quantise, ref_units
from tests.test_j_attack_gpu import _same_result, _shared
from tests.test_p_corrupt_gpu import _bits, _inputs
from tests.test_spatial_cpu import ref_warp

pytestmark = pytest.mark.gpu

SHAPES = [(n, s) for n in (1, 3) for s in (8, 20, 44, 128)]
BORDERS = ("reflect", "edge", "fill")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    ou.fit_cpu_threads()
    return torch.device("cuda:0")


def _transforms(S):
    return [dict(), dict(flip=True), dict(shift=(3, -2)), dict(shift=(0.5, 0.25)), dict(angle=90.0), dict(angle=5.0),
            dict(angle=-30.0, scale=0.8, flip=True), dict(angle=45.0, scale=1.25), dict(scale=0.5), dict(scale=0.25),
            dict(shift=(3 * S + 0.5, 3 * S + 0.5))]


def _launch(xd, mats, row, border):
    from unidefense_amd import corrupt as CR
    from unidefense_amd import kernels as K
    dev = xd.device
    mat = torch.from_numpy(np.asarray(mats, np.int64)).to(torch.int32).to(dev)
    return K.warp_affine(xd, torch.empty_like(xd), CR._lut(dev), mat, torch.tensor(row, dtype=torch.int32, device=dev), border)


@pytest.mark.parametrize("N,S", SHAPES)
def test_warp_bitwise(N, S):
    dev = _dev()
    from unidefense_amd import spatial as SP
    ts = _transforms(S)
    perm = [2, 0, 1][:N] if N == 3 else [0]
    for name, x in _inputs(N, S).items():
        u = ref_quantise(x)
        xd = torch.from_numpy(x).to(dev)
        for border in BORDERS:
            for i in range(len(ts)):
                # N = 3: the three samples take different rows of one table in one launch, through a permutation
                mats = np.array([SP.affine_q16(**ts[(i + j) % len(ts)]) for j in range(N)], np.int64)
                got = _launch(xd, mats, perm, border)
                assert torch.equal(_bits(got), _bits(ref_units(ref_warp(u, mats[perm], border)))), (name, border, i)
            # the functional form: one transform for the batch, and one per sample
            kw = ts[6]
            assert torch.equal(_bits(SP.warp(xd, border=border, **kw)), _bits(ref_units(ref_warp(u, SP.affine_q16(**kw), border))))
        if N == 3:
            got = SP.warp(xd, angle=[5.0, 0.0, -30.0], scale=[1.0, 0.5, 0.8], shift=[(0, 0), (1.5, 2), (0, -3)], flip=[False, True, False])
            mats = [SP.affine_q16(5.0), SP.affine_q16(0.0, 0.5, (1.5, 2), True), SP.affine_q16(-30.0, 0.8, (0, -3))]
            assert torch.equal(_bits(got), _bits(ref_units(ref_warp(u, mats, "reflect"))))


@pytest.mark.parametrize("N,S,kw", [(2, 256, dict(angle=17.0, scale=0.9)), (1, 380, dict(angle=-8.0, scale=1.1, shift=(4.5, -3.25)))])
def test_warp_bitwise_model_sizes(N, S, kw):
    dev = _dev()
    from unidefense_amd import spatial as SP
    x = np.random.default_rng(S).uniform(-1.0, 1.0, (N, 3, S, S)).astype(np.float32)
    xd = torch.from_numpy(x).to(dev)
    keep = xd.clone()
    out = torch.full_like(xd, 9.0)
    for border in BORDERS:
        got = SP.warp(xd, border=border, out=out, **kw)
        assert got is out
        assert torch.equal(_bits(got), _bits(ref_units(ref_warp(ref_quantise(x), SP.affine_q16(**kw), border)))), border
    assert torch.equal(_bits(xd), _bits(keep))                      # the input is left alone
    for bad in (lambda: SP.warp(xd, out=xd), lambda: SP.warp(xd[:, :2]), lambda: SP.warp(xd.double()), lambda: SP.warp(xd, angle=[1.0] * (N + 1)),
                lambda: SP.warp(xd, shift=[(0, 0)] * (N + 1)), lambda: SP.warp(xd, scale=0.0), lambda: SP.warp(xd, border="wrap")):
        with pytest.raises(ValueError):
            bad()


def test_any_table_content_stays_in_bounds():
    """The contract of ud_warp_affine: row entries outside the table are clamped, and any six int32 are a map (taps at any
    distance go through the border rule).  A bounds check of the contract on values the reference defines, not a provoked fault."""
    dev = _dev()
    from unidefense_amd import spatial as SP
    N, S = 3, 44
    x = _inputs(N, S)["noise"]
    u = ref_quantise(x)
    xd = torch.from_numpy(x).to(dev)
    ts = _transforms(S)
    mats = np.array([SP.affine_q16(**t) for t in ts[1:8]], np.int64)
    rows = mats.shape[0]
    for border in BORDERS:
        got = _launch(xd, mats, [-5, rows + 7, 3], border)
        assert torch.equal(got, _launch(xd, mats, [0, rows - 1, 3], border))
        assert torch.equal(_bits(got), _bits(ref_units(ref_warp(u, mats[[0, rows - 1, 3]], border))))
        big = 2 ** 31 - 1
        wild = np.array([[big] * 6, [-big - 1] * 6, [big, -big - 1, big, -big - 1, big, -big - 1]], np.int64)
        wild = np.concatenate([wild, np.random.default_rng(5).integers(-2 ** 31, 2 ** 31, (3, 6))], 0)
        for row in ([0, 1, 2], [3, 4, 5]):
            assert torch.equal(_bits(_launch(xd, wild, row, border)), _bits(ref_units(ref_warp(u, wild[row], border)))), (border, row)


def test_spatial_control_is_the_python_loop():
    dev = _dev()
    from unidefense_amd import kernels as K
    Kc, N = 6, 5
    nan = float("nan")
    f = torch.tensor([[3.0, 1.0, nan, -1.0, 2.0],       # column 0: ties at the minimum (k = 2 and 4 -> 2); 1: strictly falling
                      [2.5, 0.5, nan, 0.0, 2.0],        # column 2: all NaN -> k = 0 stays; 3: the minimum is at k = 0
                      [1.0, 0.25, nan, -0.5, nan],      # column 4: NaNs between values, a tie with k = 0 afterwards
                      [2.0, 0.125, nan, 5.0, 2.0],
                      [1.0, 0.0, nan, -1.0, 1.5],
                      [1.5, -0.5, nan, 7.0, nan]], dtype=torch.float32)
    ist, fst = K.spatial_state(N, dev)
    ist[K.SPATIAL_I["row"]] = torch.arange(N, dtype=torch.int32, device=dev)
    history = torch.zeros(Kc, N, device=dev)
    f_best, best_k, hist = [0.0] * N, [0] * N, torch.zeros(Kc, N)
    for k in range(Kc):
        K.spatial_control(f[k].to(dev), ist, fst, history)
        for n in range(N):                                          # the ten-line loop
            hist[k, n] = f[k, n]
            if k == 0 or float(f[k, n]) < f_best[n]:
                f_best[n], best_k[n] = float(f[k, n]), k
        row = [min(k + 1, Kc - 1) * N + n for n in range(N)]
        assert torch.equal(_bits(history), _bits(hist)), k
        assert torch.equal(_bits(fst[K.SPATIAL_F["f_best"]]), _bits(torch.tensor(f_best))), k
        assert ist[K.SPATIAL_I["best_k"]].tolist() == best_k and ist[K.SPATIAL_I["row"]].tolist() == row, k
        assert ist[K.SPATIAL_I["k"]].tolist() == [k + 1] * N
    assert best_k == [2, 5, 0, 0, 4]
    before = (ist.clone(), fst.clone(), history.clone())
    K.spatial_control(f[0].to(dev), ist, fst, history)              # a call past K writes nothing
    assert torch.equal(ist, before[0]) and torch.equal(_bits(fst), _bits(before[1])) and torch.equal(_bits(history), _bits(before[2]))
    K.spatial_control(f[0].to(dev), ist, fst, history, closing=True)
    assert ist[K.SPATIAL_I["row"]].tolist() == [b * N + n for n, b in enumerate(best_k)]
    assert ist[K.SPATIAL_I["best_k"]].tolist() == best_k and ist[K.SPATIAL_I["k"]].tolist() == [Kc] * N
    assert torch.equal(_bits(fst), _bits(before[1])) and torch.equal(_bits(history), _bits(before[2]))
    for bad in (lambda: K.spatial_control(f[0].to(dev), ist[:2].contiguous(), fst, history), lambda: K.spatial_control(f[0, :4].to(dev), ist, fst, history),
                lambda: K.spatial_control(f[0].to(dev), ist, fst, history[:, :4].contiguous()), lambda: K.spatial_control(f[0].to(dev), ist.float(), fst, history)):
        with pytest.raises(ValueError):
            bad()


# ---- the runner --------------------------------------------------------------------------------------------------------------------
RUNNER_CASES = [("UDR18", 128, 2, "fp32"), ("UDEB4", 256, 1, "fp32"), ("UDEB4", 256, 1, "fp16")]
GRID = dict(grid=(3, 2, 1))                                         # 1 + 3 * 2 * 2 = 13 candidates


def _warp_by(x, params, border="reflect"):
    """warp(x, *params) for a candidate table's rows params [N, 5] = (angle, dx, dy, scale, flip)"""
    from unidefense_amd.spatial import warp
    p = params.tolist()
    return warp(x, angle=[r[0] for r in p], scale=[r[3] for r in p], shift=[(r[1], r[2]) for r in p], flip=[r[4] != 0.0 for r in p],
                border=border)


def _snapshot(r, x_adv):
    return {"x_adv": x_adv.clone(), "history": r.history.clone(), "best_loss": r.best_loss.clone(), "best_k": r.best_k.clone(),
            "best": r.best.clone(), "loss0": r.loss0.clone()}


def _same_bits(a, b):
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k].cpu().view(torch.uint8), b[k].cpu().view(torch.uint8)), k


@pytest.mark.parametrize("name,size,n,precision", RUNNER_CASES)
def test_runner_life_cycle(name, size, n, precision):
    dev = _dev()
    from unidefense_amd import spatial as SP
    from unidefense_amd.attack import margin_each
    from unidefense_amd.infer import InferenceRunner
    m = _shared(name, dev)
    x = param_fill.make_input(n, size, 41).to(dev)
    y = param_fill.make_labels(n).to(dev)
    r = SP.SpatialRunner(m, n, size, precision=precision, **GRID)
    assert r.K == 13 and r.args == {"method": "spatial", "max_angle": 10.0, "max_shift": 0.05, "scales": (0.9, 1.1), "flip": False,
                                    "search": "grid", "grid": (3, 2, 1), "k": None, "candidates": 13, "border": "reflect",
                                    "objective": "margin", "precision": precision}
    runs = []
    for call in range(4):                                          # eager, capture, two replays
        runs.append(_snapshot(r, r(x, y)))
        assert (r.graph is not None) == (call >= 1)
    for s in runs[1:]:
        _same_bits(runs[0], s)
    s = runs[0]
    cand = SP.spatial_candidates(size, batch=n, **GRID)
    assert torch.equal(r.candidates, cand) and tuple(s["history"].shape) == (13, n)
    # the landscape is the objective of the same-precision InferenceRunner on warp(x, candidate k)
    inf = InferenceRunner(m, n, size, precision)
    inf(x)
    for k in (0, 6, 12):
        with torch.no_grad():
            f = margin_each(inf(_warp_by(x, cand[k])), y).float()
        assert torch.equal(_bits(s["history"][k]), _bits(f)), k
    h = s["history"].cpu()
    assert not torch.isnan(h).any()
    assert torch.equal(_bits(s["best_loss"]), _bits(h.min(0).values)) and torch.equal(_bits(s["loss0"]), _bits(h[0]))
    first = [int((h[:, j] == h[:, j].min()).nonzero()[0]) for j in range(n)]        # ties keep the lowest k
    assert s["best_k"].tolist() == first and s["best_k"].dtype == torch.int32
    assert s["best"].dtype == torch.float64 and torch.equal(s["best"], cand[first, torch.arange(n)])
    assert torch.equal(_bits(s["x_adv"]), _bits(_warp_by(x, s["best"])))
    assert float(h[:, 0].max()) > float(h[:, 0].min())             # the candidates do move the objective
    # a replay follows its input
    x2 = param_fill.make_input(n, size, 42).to(dev)
    s2 = _snapshot(r, r(x2, y))
    assert not torch.equal(s2["history"], s["history"])
    with torch.no_grad():
        f = margin_each(inf(_warp_by(x2, cand[12])), y).float()
    assert torch.equal(_bits(s2["history"][12]), _bits(f)) and torch.equal(_bits(s2["x_adv"]), _bits(_warp_by(x2, s2["best"])))
    _same_bits(_snapshot(r, r(x, y)), s)
    for bad in (lambda: r(x.cpu(), y), lambda: r(x[:, :, :64, :64], y), lambda: r(x.double(), y), lambda: r(x, y.int()), lambda: r(x, y.cpu())):
        with pytest.raises(ValueError):
            bad()


def test_random_search_is_reproducible_from_a_cpu_seed():
    dev = _dev()
    from unidefense_amd import spatial as SP
    n, size = 2, 128
    m = _shared("UDR18", dev)
    x = param_fill.make_input(n, size, 41).to(dev)
    y = param_fill.make_labels(n).to(dev)
    gen = lambda seed: torch.Generator().manual_seed(seed)
    r = SP.SpatialRunner(m, n, size, search="random", k=8, flip=True, border="edge", objective="cross_entropy")
    assert r.K == 9 and r.args["k"] == 8 and r.args["grid"] is None
    a = _snapshot(r, r(x, y, gen(3)))
    b = _snapshot(r, r(x, y, gen(4)))
    assert torch.equal(r.candidates, SP.spatial_candidates(size, flip=True, search="random", k=8, batch=n, generator=gen(4)))
    c = _snapshot(r, r(x, y, gen(3)))
    d = _snapshot(r, r(x, y, gen(3)))
    _same_bits(a, c)
    _same_bits(a, d)
    assert not torch.equal(a["history"][1:], b["history"][1:]) and torch.equal(_bits(a["history"][0]), _bits(b["history"][0]))
    assert torch.equal(_bits(a["x_adv"]), _bits(_warp_by(x, a["best"], "edge")))
    with pytest.raises(ValueError, match="CPU"):
        r(x, y, torch.Generator(device=dev).manual_seed(3))


def test_runner_leaves_the_model_and_the_other_runners_as_they_were():
    dev = _dev()
    from unidefense_amd import lib
    from unidefense_amd import spatial as SP
    from unidefense_amd.infer import _MAX_RUNNERS, InferenceRunner
    n, size = 2, 128
    m = _shared("UDR18", dev)
    x = param_fill.make_input(n, size, 31).to(dev)
    y = param_fill.make_labels(n).to(dev)
    flags = [p.requires_grad for p in m.parameters()]
    params = {k: v.detach().clone() for k, v in m.named_parameters()}
    bufs = {k: v.clone() for k, v in m.named_buffers()}
    slots = ("_ud_runners", "_ud_grad_runners", "_ud_attack_runners", "_ud_apgd_runners", "_ud_square_runners", "_ud_fmn_runners",
             "_ud_sparse_fmn_runners", "_ud_corruption_runners")
    caches = {k: dict(m.__dict__.get(k, {})) for k in slots}
    m.__dict__.pop("_ud_spatial_runners", None)
    inf = InferenceRunner(m, n, size)
    inf(x)
    before = inf(x)["cls_out"].clone()
    path = lib.call("ud_gemm_get_path")
    r = m.spatial_runner(n, size, **GRID)
    assert m.spatial_runner(n, size, **GRID) is r and SP.spatial_runner(m, n, size, grid=[3, 2, 1]) is r
    assert m.spatial_runner(n, size, max_angle=10.0, max_shift=0.05, scales=(0.9, 1.1), flip=False, search="grid", grid=(3, 2, 1), k=64,
                            border="reflect", objective="margin", precision="fp32") is r
    for _ in range(3):
        xa = r(x, y)
    assert torch.equal(xa, _warp_by(x, r.best))
    torch.cuda.synchronize()
    assert lib.call("ud_gemm_get_path") == path
    assert all(dict(m.__dict__.get(k, {})) == v for k, v in caches.items())
    assert [p.requires_grad for p in m.parameters()] == flags and all(p.grad is None for p in m.parameters())
    assert not m.training and not m.__dict__.get("_eval_half") and not m.__dict__.get("_eval_fused")
    assert all(torch.equal(v, params[k]) for k, v in m.named_parameters())
    now = dict(m.named_buffers())
    assert all(torch.equal(v, now[k]) for k, v in bufs.items())
    assert torch.equal(inf(x)["cls_out"], before)
    # the cache: one key per full argument tuple, _MAX_RUNNERS kept, the oldest evicted
    others = [m.spatial_runner(n, size, grid=(3, 2, 2)), m.spatial_runner(n, size, border="edge", **GRID),
              m.spatial_runner(n, size, max_angle=5.0, **GRID), m.spatial_runner(n, size, search="random", k=4)]
    cache = m.__dict__["_ud_spatial_runners"]
    assert _MAX_RUNNERS == 4 and len(cache) == 4 and len({id(o) for o in others}) == 4 and all(o is not r for o in others)
    assert m.spatial_runner(n, size, **GRID) is not r and len(cache) == 4
    m.__dict__.pop("_ud_spatial_runners", None)


def test_runner_refusals_come_before_any_kernel():
    dev = _dev()
    from tests.test_spatial_cpu import BAD
    from unidefense_amd import spatial as SP
    from unidefense_amd.model import load_model
    m = _shared("UDR18", dev)
    m.__dict__.pop("_ud_spatial_runners", None)
    for kw, match in BAD:
        for make in (lambda: SP.SpatialRunner(m, 2, 64, **kw), lambda: m.spatial_runner(2, 64, **kw)):
            with pytest.raises(ValueError, match=match):
                make()
    assert not m.__dict__.get("_ud_spatial_runners")
    m.train()
    try:
        with pytest.raises(ValueError, match="eval"):
            m.spatial_runner(2, 64)
    finally:
        m.eval()
    r = m.spatial_runner(2, 64, **GRID)
    y = torch.zeros(2, dtype=torch.int64, device=dev)
    m.train()
    try:
        with pytest.raises(ValueError, match="training"):
            r(torch.zeros(2, 3, 64, 64, device=dev), y)
    finally:
        m.eval()
    for bad in (lambda: r(torch.zeros(2, 3, 64, 64), y), lambda: r(torch.zeros(2, 3, 32, 32, device=dev), y),
                lambda: r(torch.zeros(2, 3, 64, 64, device=dev), y[:1])):
        with pytest.raises(ValueError):
            bad()
    assert r.calls == 0 and r.x0 is None and r.x_adv is None and r.history is None and r.graph is None
    with pytest.raises(ValueError, match="cuda"):
        SP.SpatialRunner(load_model("UDR18")(num_classes=2).eval(), 2, 64)
    m.__dict__.pop("_ud_spatial_runners", None)


# ---- the engine --------------------------------------------------------------------------------------------------------------------
def test_engine_test_spatial():
    _dev()
    from tests.test_d_train_engine import CONFIG
    from unidefense_amd.attack import margin_each
    from unidefense_amd.engine import get_engine
    torch.manual_seed(0)
    eng = get_engine("FE")(copy.deepcopy(CONFIG), "Test")
    t0 = eng.test(1)
    a = eng.test_spatial(batches=1, spatial={"grid": (3, 2, 1)})
    b = eng.test_spatial(batches=1, spatial={"grid": (3, 2, 1)})
    assert set(a) == {"clean", "adv", "attack"}
    _same_result(a["clean"], t0)
    _same_result(b["clean"], t0)
    _same_result(a["adv"], b["adv"])
    assert set(a["adv"]) == set(t0) and torch.equal(a["adv"]["labels"], t0["labels"])
    best = a["attack"]["best"]
    n = t0["labels"].numel()
    assert best.device.type == "cpu" and tuple(best.shape) == (n, 5) and torch.equal(best, b["attack"]["best"])
    assert a["attack"]["candidates"] == 13 and a["attack"]["grid"] == (3, 2, 1) and a["attack"]["method"] == "spatial"
    assert {k: v for k, v in a["attack"].items() if k not in ("best", "fooled")} == {k: v for k, v in b["attack"].items() if k not in ("best", "fooled")}
    # "adv" scores warp(x, *best) with the eager model; "fooled" is the runner's losses
    xr, yr, xf, yf = eng.test_iterator(1, eng.batch, eng.size, eng.device)
    x, y = torch.cat([xr, xf], 0).contiguous(), torch.cat([yr, yf], 0)
    with torch.no_grad():
        want = torch.softmax(eng.model(_warp_by(x, best))["cls_out"], 1)[:, 0]
    assert torch.equal(a["adv"]["scores"], want.cpu())
    runner = eng.model_without_ddp.spatial_runner(x.shape[0], x.shape[-1], grid=(3, 2, 1))
    runner(x, y)
    held = runner.loss0 > 0
    fooled = float((runner.best_loss[held] <= 0).double().mean()) if bool(held.any()) else float("nan")
    assert a["attack"]["fooled"] == fooled or (fooled != fooled and a["attack"]["fooled"] != a["attack"]["fooled"])
    assert a["attack"]["fooled"] == b["attack"]["fooled"] or fooled != fooled
    with torch.no_grad():
        assert bool((runner.best_loss <= runner.loss0).all())
    # a random search takes its seed from the dict
    c = eng.test_spatial(batches=1, spatial={"search": "random", "k": 4, "seed": 5})
    d = eng.test_spatial(batches=1, spatial={"search": "random", "k": 4, "seed": 5})
    assert torch.equal(c["attack"]["best"], d["attack"]["best"]) and c["attack"]["candidates"] == 5
    _same_result(c["adv"], d["adv"])
    for bad in ({"search": "sobol"}, {"grid": (0, 1, 1)}, {"border": "wrap"}, {"angle": 3.0}, {"scales": (1.2, 0.8)}):
        with pytest.raises(ValueError):
            eng.test_spatial(batches=1, spatial=bad)
    with pytest.raises(ValueError, match="method"):
        eng.test_robust(batches=1, attack={"method": "spatial", "eps": 0.1})
    _same_result(eng.test(1), t0)
