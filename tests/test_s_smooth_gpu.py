"""GPU: randomized smoothing's kernels (csrc/smooth.hip), CertifyRunner (unidefense_amd/smooth.py) and
TrainEngine.test_certified.

Kernels: the uniform noise bitwise against the numpy restatement, the Gaussian noise against its float64 restatement (bar: three
times what the OpenCL full-profile ULP limits of log, sqrt and sinpi / cospi give at |z| = 5.77), position independence bitwise,
the vote exactly.  Runner: exact end-to-end counts with a known classifier (the recorded restatement of
tools/smooth_fixture.py), the life cycle (eager, capture, replay) on real forwards with every draw re-created by
runner.noise, and the stage."""
import copy
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle import param_fill
from tests.margins import within
from tests.test_j_attack_gpu import _dev, _shared
from unidefense_amd import smooth as S

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 75), (4, 192), (5, 4097), (33, 3072)]     # scalar path, vector path, a tail, more than one block, many samples
OFFSET = (4, 192, True)                                          # a vector shape from a base one float off 16 bytes: scalar path
KERNEL_CASES = [s + (False,) for s in SHAPES] + [OFFSET]
SEED = (0x5EED << 32) | 20261020                                 # a non-zero high word
BIG_ID = (1 << 32) + 9


def _place(t, dev, offset):
    """t on the device; offset: inside a larger buffer, one float behind a 16-byte boundary"""
    if not offset:
        return t.to(dev).contiguous()
    big = torch.zeros(t.numel() + 1, dtype=t.dtype, device=dev)
    out = big[1:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


def _bits(t):
    return (t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)).view(np.uint32)


def _ids(N):
    ids = torch.arange(N, dtype=torch.int64) * 3 + 1
    ids[N // 2] = BIG_ID
    return ids


def _case(N, per):
    gen = torch.Generator().manual_seed(N * 131 + per)
    x = torch.rand(N, per, generator=gen) * 2 - 1
    k = torch.randint(0, 1000, (N,), generator=gen, dtype=torch.int32)
    return x, _ids(N), k


# ---- 1. uniform noise: bitwise -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,per,offset", KERNEL_CASES)
def test_uniform_noise_bitwise_vs_restatement(N, per, offset):
    from unidefense_amd import kernels as K
    dev = _dev()
    x, ids, k = _case(N, per)
    lam = float(np.float32(math.sqrt(3.0) * 0.25))
    xd, idd, kd = _place(x, dev, offset), ids.to(dev), k.to(dev)
    for draw0, kk in ((5, None), (0, k), (17, k)):                   # the draw from draw0 alone, from k alone, from both
        out = _place(torch.full((N, per), 9.0), dev, offset)
        got = K.smooth_noise(xd, out, idd, None if kk is None else kd, draw0, "uniform", lam, SEED)
        torch.cuda.synchronize()
        assert got is out and torch.equal(xd.cpu(), x)               # x is only read
        want = S.ref_smooth_noise(x, ids, draw0 + (0 if kk is None else kk.numpy().astype(np.int64)), "uniform", lam, SEED)
        assert want.dtype == np.float32 and np.array_equal(_bits(got), _bits(want)), (N, per, draw0)
    assert not np.array_equal(_bits(got), _bits(x))
    # out is x
    again = _place(x, dev, offset)
    assert K.smooth_noise(again, again, idd, kd, 17, "uniform", lam, SEED) is again and np.array_equal(_bits(again), _bits(want))
    # scale = 0 returns x bitwise
    assert np.array_equal(_bits(K.smooth_noise(xd, out, idd, kd, 3, "uniform", 0.0, SEED)), _bits(x))
    # a NaN in x shows at its element only
    n, e = N // 2, per // 2
    bad = x.clone()
    bad[n, e] = float("nan")
    got = K.smooth_noise(_place(bad, dev, offset), out, idd, kd, 17, "uniform", lam, SEED).cpu()
    keep = torch.ones(N, per, dtype=torch.bool)
    keep[n, e] = False
    assert bool(torch.isnan(got[n, e])) and np.array_equal(_bits(got[keep]), _bits(torch.from_numpy(want)[keep]))


# ---- 2. Gaussian noise -------------------------------------------------------------------------------------------------------------
Z_BAR = 1e-5          # 3 x (5.77 x ~9.5 ulp = 3.3e-6): log 3 ulp, sqrt 3 ulp, sinpi / cospi 4 ulp, the product's rounding


@pytest.mark.parametrize("N,per,offset", KERNEL_CASES)
def test_gaussian_noise_vs_float64_restatement(N, per, offset):
    from unidefense_amd import kernels as K
    dev = _dev()
    x, ids, k = _case(N, per)
    idd, kd = ids.to(dev), k.to(dev)
    zero = _place(torch.zeros(N, per), dev, offset)
    z = K.smooth_noise(zero, _place(torch.full((N, per), 9.0), dev, offset), idd, kd, 2, "gaussian", 1.0, SEED).cpu()
    ref = S.ref_smooth_noise(torch.zeros(N, per), ids, 2 + k.numpy().astype(np.int64), "gaussian", 1.0, SEED)
    assert ref.dtype == np.float64 and float(np.abs(ref).max()) <= math.sqrt(48 * math.log(2))
    err = float(np.abs(z.numpy().astype(np.float64) - ref).max())
    print(f"  gaussian N {N} per {per} offset {offset}: max |z_gpu - z_ref64| {err:.3e}  max |z| {float(z.abs().max()):.3f}")
    assert within(f"smooth gaussian z N{N} per{per}", err, Z_BAR)
    # x != 0: one fp32 product and one fp32 add on the same z
    scale = np.float32(0.37)
    got = K.smooth_noise(_place(x, dev, offset), _place(torch.zeros(N, per), dev, offset), idd, kd, 2, "gaussian", float(scale), SEED)
    want = (x.numpy() + (scale * z.numpy()).astype(np.float32)).astype(np.float32)
    assert np.array_equal(_bits(got), _bits(want))


# ---- 3. position independence on the device: bitwise -------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", S.NOISES)
def test_noise_does_not_depend_on_the_row_or_the_path(mode):
    from unidefense_amd import kernels as K
    dev = _dev()
    per = 192
    gen = torch.Generator().manual_seed(3)
    x = torch.rand(5, per, generator=gen) * 2 - 1
    ids = torch.tensor([1, 2, BIG_ID, 7, 9])
    k = torch.tensor([4, 0, 9, 6, 2], dtype=torch.int32)
    full = K.smooth_noise(x.to(dev), torch.empty(5, per, device=dev), ids.to(dev), k.to(dev), 1, mode, 0.5, SEED).cpu()
    # the sample with id 7 alone, in an N = 1 launch, with its draw given by draw0
    alone = K.smooth_noise(x[3:4].to(dev), torch.empty(1, per, device=dev), ids[3:4].to(dev), None, 7, mode, 0.5, SEED).cpu()
    assert np.array_equal(_bits(alone[0]), _bits(full[3]))
    # the vector and the scalar path: the same buffer one float off 16 bytes, and a shorter sample that ends inside a quad
    off = K.smooth_noise(_place(x, dev, True), _place(torch.zeros(5, per), dev, True), ids.to(dev), k.to(dev), 1, mode, 0.5, SEED)
    assert np.array_equal(_bits(off), _bits(full))
    short = K.smooth_noise(x[:, :190].contiguous().to(dev), torch.empty(5, 190, device=dev), ids.to(dev), k.to(dev), 1, mode, 0.5, SEED)
    assert np.array_equal(_bits(short), _bits(full[:, :190].contiguous()))
    # another seed, id or draw: another field
    for other in (K.smooth_noise(x.to(dev), torch.empty(5, per, device=dev), ids.to(dev), k.to(dev), 1, mode, 0.5, SEED + 1),
                  K.smooth_noise(x.to(dev), torch.empty(5, per, device=dev), ids.to(dev), k.to(dev), 2, mode, 0.5, SEED),
                  K.smooth_noise(x.to(dev), torch.empty(5, per, device=dev), (ids + 1).to(dev), k.to(dev), 1, mode, 0.5, SEED)):
        assert float((other.cpu() != full).double().mean()) > 0.99


# ---- 4. ud_smooth_vote: exact --------------------------------------------------------------------------------------------------------
VALUES = torch.tensor([float("-inf"), -1.0, 0.0, 0.0, 0.5, 0.5, 2.0, float("inf")])


@pytest.mark.parametrize("start", ["zero", "boundary", "done", "mixed"])
@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("N", [1, 5, 300])
def test_vote_exact_vs_restatement(N, C, start):
    from unidefense_amd import kernels as K
    dev = _dev()
    draws, n0 = 6, 3
    gen = torch.Generator().manual_seed(N * 7 + C)
    ist, counts, votes, margins = K.smooth_state(N, draws, C, dev)
    assert tuple(counts.shape) == (2, N, max(C, 2)) and tuple(votes.shape) == (draws, N) == tuple(margins.shape)
    k0 = {"zero": torch.zeros(N), "boundary": torch.full((N,), n0 - 1), "done": torch.full((N,), draws),
          "mixed": torch.arange(N) % (draws + 3) - 1}[start].to(torch.int32)
    ist[K.SMOOTH_I["k"]].copy_(k0)
    votes.fill_(-7)
    margins.fill_(-7.0)
    rk, rc = k0.numpy().copy(), np.zeros((2, N, max(C, 2)), dtype=np.int32)
    rv, rm = np.full((draws, N), -7, dtype=np.int32), np.full((draws, N), -7.0, dtype=np.float32)
    for launch in range(3):                                      # three draws: from n0 - 1 they cross the phase boundary
        logits = VALUES[torch.randint(0, len(VALUES), (N, C), generator=gen)]      # ties and infinities
        logits[launch % N] = float("nan") if C == 1 else torch.tensor([float("nan")] + [1.0] * (C - 1))[torch.randperm(C, generator=gen)]
        K.smooth_vote(logits.to(dev), ist, counts, votes, margins, n0)
        S.ref_smooth_vote(logits.numpy(), rk, rc, rv, rm, n0)
    torch.cuda.synchronize()
    assert np.array_equal(ist.cpu().numpy()[0], rk) and np.array_equal(counts.cpu().numpy(), rc)
    assert np.array_equal(votes.cpu().numpy(), rv)
    gm = margins.cpu().numpy()
    assert np.array_equal(np.isnan(gm), np.isnan(rm)) and np.array_equal(gm[~np.isnan(rm)], rm[~np.isnan(rm)])
    if start == "done":
        assert not rc.any() and (rv == -7).all()                 # a counter outside the range writes nothing
    if start == "boundary" and N > 1:
        assert rc[0].sum() > 0 and rc[1].sum() > 0               # the run crossed the phase boundary


# ---- 5. exact end-to-end counts with a known classifier -----------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smooth_counts_n5.npz")


def test_exact_counts_with_a_known_classifier():
    """UDR18 at 128 x 128, N = 5, uniform noise, sigma 0.25, n0 = 32, n = 512, alpha = 0.001; the classifier is the hook
    (mean(x_noisy) - t_n, 0).  The recorded means are ref_smooth_noise's (tools/smooth_fixture.py chose the seed and the
    thresholds so that no |mean - t| is below 1e-5); a few draws of every sample are recomputed here and must be the recorded
    ones bit for bit.  Everything the runner leaves must then be what float64 host math makes of those means."""
    from tests.smooth_case import ALPHA, N0, NE, SIGMA, SIZE, decide, restated_means
    dev = _dev()
    g = np.load(GOLDEN)
    seed, ids, t, p_true, means = int(g["seed"]), g["ids"], g["t"], g["p_true"], g["means"]
    N = len(ids)
    assert (N, SIZE, SIGMA, N0, NE, ALPHA) == (5, 128, 0.25, 32, 512, 0.001) and means.shape == (N, N0 + NE) and t.dtype == np.float32
    x = param_fill.make_input(N, SIZE, int(g["input_seed"]))
    some = [0, N0 - 1, N0, N0 + NE - 1]
    assert np.array_equal(restated_means(x.numpy(), ids, some, seed), means[:, some])
    clear = float(np.abs(means - t.astype(np.float64)[:, None]).min())
    assert clear >= 1e-5                                         # no vote is exempt: none is within the reduction's rounding
    votes, counts0, counts, ca, predicted, p_lower, radius = decide(means, t)
    # soundness on these inputs, first on the CPU: the bound is below the selected class's true vote probability
    assert bool((p_lower <= np.where(ca == 0, p_true, 1.0 - p_true)).all())
    assert predicted.tolist() == [0, 0, 0, -1, 1] and [round(float(p), 1) for p in p_true] == [1.0, 0.9, 0.7, 0.5, 0.1]

    td = torch.from_numpy(t).to(dev)
    r = S.CertifyRunner(_shared("UDR18", dev), N, SIZE, sigma=SIGMA, noise="uniform", n0=N0, n=NE, alpha=ALPHA, seed=seed,
                        logits=lambda out, xn: torch.stack([xn.mean((1, 2, 3)) - td, torch.zeros_like(td)], 1))
    xd, idd = x.to(dev), torch.from_numpy(ids).to(dev)
    for call in range(3):                                        # eager, capture + replay, replay
        got = r(xd, idd)
        assert (r.graph is None) == (call == 0)
        gm = r.margins.cpu().numpy().astype(np.float64)
        dev_err = float(np.abs(gm - np.abs(means.T - t.astype(np.float64)[None, :])).max())
        print(f"  call {call}: max | |mean - t| device - restatement | {dev_err:.3e}  clearance {clear:.3e}")
        assert within("smooth mean vs restatement", dev_err, clear / 40)
        assert np.array_equal(r.votes.cpu().numpy(), votes), call
        assert np.array_equal(r.counts0.cpu().numpy(), counts0) and np.array_equal(r.counts.cpu().numpy(), counts)
        assert r.predicted.dtype == torch.int64 and r.predicted.tolist() == predicted.tolist()
        assert r.p_lower.dtype == torch.float64 and float(np.abs(r.p_lower.cpu().numpy() - p_lower).max()) <= 1e-9
        assert got is r.radius and got.dtype == torch.float32 and tuple(got.shape) == (N,)
        assert bool(np.all(np.abs(got.cpu().numpy().astype(np.float64) - radius) <= 1e-6 * radius))
        assert bool((r.p_lower.cpu().numpy() <= np.where(ca == 0, p_true, 1.0 - p_true)).all())
        assert int(r.predicted[3]) == -1 and float(got[3]) == 0.0 and int(r.predicted[4]) == 1 and float(got[4]) > 0.0
    assert r.args["method"] == "certify" and r.args["norm"] == "l1" and r.args["noise"] == "uniform"
    # the draw the certificate saw, re-created alone: x_noisy holds the last draw
    last = r.noise(xd[1:2], idd[1:2], draw=N0 + NE - 1)
    assert torch.equal(last[0], r.x_noisy[1])


# ---- 6. life cycle and real forwards ------------------------------------------------------------------------------------------------
CASES = [("UDR18", 128, 2, 5, "fp32"), ("UDEB4", 256, 1, 7, "fp32"), ("UDEB4", 256, 1, 7, "fp16")]
KEEP = ("radius", "predicted", "p_lower", "counts0", "counts", "votes", "margins")
N0_LC, N_LC, ALPHA_LC = 3, 5, 0.5          # alpha 0.5: five unanimous draws certify (0.5^(1/5) = 0.87); at 0.001 five draws never could


@functools.lru_cache(maxsize=None)
def _certified(name, size, n, seed, precision, noise):
    """the eager first call, then two replays; shared by the tests below and left unchanged"""
    dev = _dev()
    m = _shared(name, dev)
    x = param_fill.make_input(n, size, seed).to(dev)
    ids = torch.arange(n, dtype=torch.int64) + 40
    r = S.CertifyRunner(m, n, size, sigma=0.25, noise=noise, n0=N0_LC, n=N_LC, alpha=ALPHA_LC, seed=SEED, precision=precision)
    snap = lambda: {k: getattr(r, k).clone() for k in KEEP}      # noqa: E731
    r(x, ids)
    assert r.graph is None and r.calls == 1
    warm = snap()
    runs = []
    for _ in range(2):
        r(x, ids)
        runs.append(snap())
    torch.cuda.synchronize()
    assert r.graph is not None
    return {"runner": r, "x": x, "ids": ids, "warm": warm, "runs": runs}


@pytest.mark.parametrize("noise", S.NOISES)
@pytest.mark.parametrize("name,size,n,seed,precision", CASES)
def test_runner_life_cycle_and_what_it_leaves(name, size, n, seed, precision, noise):
    a = _certified(name, size, n, seed, precision, noise)
    r, draws = a["runner"], N0_LC + N_LC
    assert r.args == {"method": "certify", "norm": S.NORM_OF[noise], "sigma": 0.25, "noise": noise, "n0": N0_LC, "n": N_LC,
                      "alpha": ALPHA_LC, "seed": SEED, "logits": None, "precision": precision}
    for k in KEEP:                                               # two replays are bitwise equal, and equal the eager first call
        assert torch.equal(a["runs"][0][k], a["runs"][1][k]), k
        assert torch.equal(a["runs"][0][k], a["warm"][k]), k
    s = a["runs"][0]
    assert tuple(s["votes"].shape) == (draws, n) == tuple(s["margins"].shape) and s["votes"].dtype == torch.int32
    assert tuple(s["counts0"].shape) == (n, 2) == tuple(s["counts"].shape) and s["counts"].dtype == torch.int32
    assert bool(((s["votes"] == 0) | (s["votes"] == 1)).all()) and bool((s["margins"] >= 0).all())
    assert s["counts0"].sum(1).tolist() == [N0_LC] * n and s["counts"].sum(1).tolist() == [N_LC] * n
    assert r.ist[0].tolist() == [draws] * n
    votes = s["votes"].cpu().numpy()
    for c in (0, 1):
        assert (votes[:N0_LC] == c).sum(0).tolist() == s["counts0"][:, c].tolist()
        assert (votes[N0_LC:] == c).sum(0).tolist() == s["counts"][:, c].tolist()
    # the host tail on those counts
    for i in range(n):
        ca = int(int(s["counts0"][i, 1]) > int(s["counts0"][i, 0]))                # n0 is odd: no tie
        p = S.clopper_pearson_lower(int(s["counts"][i, ca]), N_LC, ALPHA_LC)
        assert float(s["p_lower"][i]) == p and int(s["predicted"][i]) == (ca if p > 0.5 else -1)
        assert float(s["radius"][i]) == float(S.certified_radius(p, 0.25, noise).float())
        assert (float(s["radius"][i]) > 0) == (p > 0.5)
    assert set(r.out) >= {"cls_out"} and tuple(r.out["cls_out"].shape) == (n, 2)
    m = r.model
    assert not m.training and all(p.grad is None for p in m.parameters())


@pytest.mark.parametrize("name,size,n,seed,precision", CASES)
def test_every_draw_can_be_recreated_alone(name, size, n, seed, precision):
    """runner.noise(x, ids, draw) gives the draw's input back: the eval forward on it votes as the certificate recorded, with
    the recorded margin (the same batch composition: the same bits)"""
    from unidefense_amd.infer import _eval_nodes
    a = _certified(name, size, n, seed, precision, "gaussian")
    r, x, ids = a["runner"], a["x"], a["ids"]
    assert torch.equal(r.noise(x, ids, draw=N0_LC + N_LC - 1), r.x_noisy)              # the last draw is still in the buffer
    worst = 0.0
    for d in (0, N0_LC - 1, N0_LC, N0_LC + N_LC - 1):
        xn = r.noise(x, ids, draw=d)
        assert not torch.equal(xn, x) and float((xn - x).std()) == pytest.approx(0.25, rel=0.02)
        with torch.no_grad(), _eval_nodes(r.model, r.half):
            z = r.model(xn)["cls_out"].float()
        top = z.sort(1, descending=True).values
        assert z.argmax(1).to(torch.int32).tolist() == a["runs"][0]["votes"][d].tolist(), d
        worst = max(worst, float(((top[:, 0] - top[:, 1]) - a["runs"][0]["margins"][d]).abs().max()))
    print(f"  {name} {precision}: max |margin re-created - recorded| {worst:.3e}")
    assert within(f"smooth margin re-created {name} {precision}", worst, 0.0)
    # other ids: another noise field, hence other margins
    r2 = S.CertifyRunner(r.model, n, size, sigma=0.25, n0=1, n=1, alpha=ALPHA_LC, seed=SEED, precision=precision)
    r2(x, ids + 1)
    assert not torch.equal(r2.margins[0], a["runs"][0]["margins"][0])
    r2(x, ids)
    assert torch.equal(r2.margins[0], a["runs"][0]["margins"][0]) and torch.equal(r2.votes[0], a["runs"][0]["votes"][0])


def test_runner_refuses_bad_inputs_and_counts_nan_rows_as_misses():
    dev = _dev()
    m = _shared("UDR18", dev)
    x = param_fill.make_input(2, 128, 5).to(dev)
    nan_row = torch.tensor([[float("nan"), 0.0], [1.0, 0.0]], device=dev)
    r = S.CertifyRunner(m, 2, 128, n0=2, n=4, alpha=ALPHA_LC, logits=lambda out, xn: nan_row)
    for bad, text in ((x.cpu(), "cuda"), (x[:1], "differs from the runner's key"), (x.double(), "differs from the runner's key")):
        with pytest.raises(ValueError, match=text):
            r(bad)
    for ids in (torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), [0, 1]):
        with pytest.raises(ValueError, match="ids must be an int64 tensor"):
            r(x, ids)
    assert r.calls == 0
    for _ in range(3):
        radius = r(x)
        assert r.votes[:, 0].tolist() == [-1] * 6 and bool(torch.isnan(r.margins[:, 0]).all())      # votes for nobody
        assert r.counts0[0].tolist() == [0, 0] and r.counts[0].tolist() == [0, 0]
        assert int(r.predicted[0]) == -1 and float(radius[0]) == 0.0 and float(r.p_lower[0]) == 0.0  # every draw missed
        assert r.counts[1].tolist() == [4, 0] and int(r.predicted[1]) == 0 and float(radius[1]) > 0
    with pytest.raises(ValueError, match=r"is no \[n, 3, 128, 128\] torch.float32 batch"):
        r.noise(x[:, :, :64])
    with pytest.raises(ValueError, match="draw must be an integer"):
        r.noise(x, draw=-1)
    with pytest.raises(ValueError, match=r"logits must be a \[2, C\] tensor"):
        S.CertifyRunner(m, 2, 128, n0=1, n=1, logits=lambda out, xn: nan_row[0])(x)
    out = torch.empty_like(x)
    assert r.noise(x, out=out) is out and torch.equal(out, r.noise(x, torch.arange(2), 0))
    assert torch.equal(r.noise(x[1:], torch.tensor([1])), out[1:])                     # any n, any row


# ---- 7. the stage ---------------------------------------------------------------------------------------------------------------------
def test_engine_test_certified():
    _dev()
    from tests.test_d_train_engine import CONFIG
    from unidefense_amd.engine import get_engine
    cfg = copy.deepcopy(CONFIG)
    cfg["model"] = {"name": "UDR18", "num_classes": 2, "drop_rate": 0.2}
    cfg["data"] = {"train_batch_size": 2, "size": 128}
    cfg["config"]["certify"] = {"sigma": 0.125, "n0": 2, "n": 6, "alpha": 0.25, "seed": 3}
    eng = get_engine("FE")(cfg, "Test")
    param_fill.fill_module_(eng.model_without_ddp, sf_coef=0.0, fuse_coef=0.3)
    with pytest.raises(ValueError, match="certify takes CertifyRunner's keyword arguments and 'grid'"):
        eng.test_certified(batches=1, certify={"sigma": 0.125, "stepz": 3})
    res = eng.test_certified(batches=2)
    assert set(res) == {"clean", "certify"}
    c = res["certify"]
    assert set(c) == {"args", "radius", "predicted", "abstained", "accuracy", "median_radius", "grid", "certified_accuracy"}
    assert c["args"]["method"] == "certify" and c["args"]["norm"] == "l2" and c["args"]["sigma"] == 0.125 and c["args"]["n"] == 6
    assert tuple(c["radius"].shape) == (8,) == tuple(c["predicted"].shape) and c["radius"].device.type == "cpu"
    assert c["grid"].tolist() == [0.0625 * i for i in range(9)] and tuple(c["certified_accuracy"].shape) == (9,)
    labels = res["clean"]["labels"]
    assert c["accuracy"] == float((c["predicted"] == labels).double().mean())
    assert c["abstained"] == float((c["predicted"] == -1).double().mean())
    assert bool(((c["radius"] > 0) == (c["predicted"] >= 0)).all())
    assert torch.equal(c["certified_accuracy"], S.certified_curve(c["radius"], c["predicted"], labels, c["grid"]))
    assert float(c["certified_accuracy"][0]) <= c["accuracy"] and bool((c["certified_accuracy"].diff() <= 0).all())
    # the clean column is test()'s; batch b's sample i drew the stream 4 b + i: the second batch alone, with those ids, certifies alike
    assert torch.equal(res["clean"]["scores"], eng.test(batches=2)["scores"])
    runner = eng.model_without_ddp.certify_runner(4, 128, **cfg["config"]["certify"])
    x = torch.cat([t for t in eng._evaluator().iterator(2, 2, 128, runner.device)[0::2]], 0).contiguous()
    assert torch.equal(runner(x, torch.arange(4, 8)).cpu(), c["radius"][4:])
    assert all(p.grad is None for p in eng.model_without_ddp.parameters())
