"""UniDefenseModelRes18 (BASELINE configs[0]: ResNet18 backbone, 128x128, bs 8).
CPU: the oracle restatement (oracle/r18.py) vs the vectors recorded from the REFERENCE (tests/golden/udr18_n8.npz).
GPU: the HIP model and its new operators vs those vectors and vs the oracle in float64."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import losses as OL
from oracle import param_fill, r18
from tests import oracle_util as ou
from tests.margins import within

GRAD_RTOL, GRAD_ATOL = 1e-3, 2e-5


def make_rng_r18(n, seed, drop_rate=0.5):
    g = torch.Generator().manual_seed(seed)

    def bern(shape, keep):
        return (torch.rand(shape, generator=g) < keep).float()
    return {"dec_keep": bern((n, 448, 16, 16), 0.8), "emb_keep": bern((n, 512, 8, 8), 1.0 - drop_rate),
            "feat_keep": bern((n, 512), 1.0 - drop_rate)}


def r18_state(dtype=torch.float32, requires_grad=False):
    sd = param_fill.fill_state_dict(r18.r18_state_shapes(2), 0.0, 0.3, dtype)
    if requires_grad:
        for k, v in sd.items():
            if v.dtype.is_floating_point and not k.endswith(("running_mean", "running_var")) and k != "bottleneck.bias":
                v.requires_grad_(True)
    return sd


def _rel(a, b):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _check_outputs(out, g, prefix, tol):
    ld = out["loss_dict"]
    pairs = [("cls_out", out["cls_out"]), ("rec_pool8", F.adaptive_avg_pool2d(out["rec"].detach().cpu(), 8)),
             ("factorization", ld["factorization"][:, :64])]
    pairs += [(k, ld[k]) for k in ("freq_mask", "spat_mask", "spatial", "freq")]
    pairs += [(f"triplet{i}", t) for i, t in enumerate(ld["triplet"])]
    bad = []
    for k, v in pairs:
        e = _rel(v, g[prefix + k])
        print(f"  {k}: rel err {e:.3e}")
        if not within(prefix + k, e, tol):
            bad.append((k, e))
    assert not bad, bad


def _loss(out, tgt, lam, losses_mod=None):
    return OL.pass1_loss(out, tgt, len(tgt) // 2, len(tgt) // 2, lam)["total_loss"]


# ------------------------------------------------------------------------------------------------ CPU
def test_oracle_r18_matches_reference_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "udr18_n8.npz"))
    n, size, seed, mseed = [int(v) for v in g["meta"]]
    x = param_fill.make_input(n, size, seed)
    tgt = param_fill.make_labels(n)
    rng = make_rng_r18(n, mseed)
    sd = r18_state()
    with torch.no_grad():
        _check_outputs(r18.forward_r18(sd, x, training=False), g, "eval_", 2e-5)
    for variant, lam in (("full", ou.LAMBDAS), ("smooth", ou.SMOOTH_LAMBDAS)):
        sd = r18_state(requires_grad=True)
        out = r18.forward_r18(sd, x, training=True, drop_rate=0.5, rng=rng)
        if variant == "full":
            _check_outputs(out, g, "train_", 5e-5)
        total = _loss(out, tgt, lam)
        assert abs(total.item() - float(g[f"{variant}_loss_total_loss"])) <= 2e-5 * abs(float(g[f"{variant}_loss_total_loss"]))
        total.backward()
        # the scalar sf_coef gradients are global sums with heavy cancellation: two fp32 evaluations that only differ in op
        # grouping disagree at the 1e-2 level on the small ones, by how much depends on the CPU's kernels — they are held in
        # float64 on both sides (the float64 oracle vs the reference run in float64)
        sd64 = r18_state(torch.float64, requires_grad=True)
        _loss(r18.forward_r18(sd64, x.double(), training=True, drop_rate=0.5, rng=rng), tgt, lam).backward()
        for i, k in enumerate(str(s) for s in g["grad_names"]):
            f64 = k.endswith("sf_coef")
            rn = float(g[f"{'f64_' if f64 else ''}{variant}_grad_norms"][i])
            tol = 1e-7 * rn + 1e-12 if f64 else GRAD_RTOL * rn + GRAD_ATOL
            gr = (sd64 if f64 else sd)[k].grad
            head = gr.flatten()[:8].numpy()
            err = max(abs(gr.double().norm().item() - rn),
                      float(np.abs(head - g[f"{'f64_' if f64 else ''}{variant}_grad_heads"][i][: head.size]).max()))
            assert err < tol, (variant, k, err, tol)


# ------------------------------------------------------------------------------------------------ GPU
def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def to_pix(t):
    return t.permute(0, 2, 3, 1).contiguous()


def to_nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


@pytest.mark.gpu
def test_resnet_operators():
    """conv (7x7/2, 3x3/2, 1x1/2) with data + weight gradients, BN+ReLU, max-pool, avg-pool, add+ReLU, concat."""
    dev = _dev()
    from tests.test_a_kernels_gpu import check_all, grads, rnd, run_tape
    from unidefense_amd import tape as T
    N = 2
    for (Ci, Co, k, s, p, H, need_dx) in ((3, 64, 7, 2, 3, 32, False), (64, 128, 3, 2, 1, 32, True),
                                          (64, 128, 1, 2, 0, 32, True), (448, 512, 3, 2, 1, 16, True)):
        x, w = rnd(N, Ci, H, H, seed=1), rnd(Co, Ci, k, k, seed=2, scale=0.1)
        Ho = (H + 2 * p - k) // s + 1
        gy = rnd(N, Co, Ho, Ho, seed=3)

        def ref(dt):
            xr, wr = x.to(dt).requires_grad_(), w.to(dt).requires_grad_()
            yr = F.conv2d(xr, wr, None, s, p)
            return dict(zip((f"conv k{k} s{s} y", f"conv k{k} s{s} dx", f"conv k{k} s{s} dw"),
                            [yr.detach()] + grads(yr, [xr, wr], gy)))
        outs, gin, gp = run_tape(lambda t, a, b: T.conv_dense_any(t, a, b, s, p, need_dx=need_dx), [to_pix(x).to(dev)],
                                 [w.to(dev)], lambda o: [to_pix(gy).to(dev)])
        got = {f"conv k{k} s{s} y": to_nchw(outs[0]), f"conv k{k} s{s} dw": gp[0]}
        if need_dx:
            got[f"conv k{k} s{s} dx"] = to_nchw(gin[0])
        check_all(got, ref)
    # BN + ReLU
    C, H = 128, 16
    x = rnd(N, C, H, H, seed=1) + 0.2
    g_, b_ = rnd(C, seed=2) * 0.1 + 1, rnd(C, seed=3) * 0.1
    gy = rnd(N, C, H, H, seed=4)

    def ref(dt):
        xr, gr, br = x.to(dt).requires_grad_(), g_.to(dt).requires_grad_(), b_.to(dt).requires_grad_()
        yr = F.relu(F.batch_norm(xr, None, None, gr, br, True, 0.1, 1e-5))
        return dict(zip(("bn-relu y", "bn-relu dx", "bn-relu dgamma"), [yr.detach()] + grads(yr, [xr, gr], gy)))
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    outs, gin, gp = run_tape(lambda t, a, w_, bb: T.batchnorm_act(t, a, w_, bb, rm, rv, 1e-5, 0.1, True, 2),
                             [to_pix(x).to(dev)], [g_.to(dev).requires_grad_(), b_.to(dev).requires_grad_()],
                             lambda o: [to_pix(gy).to(dev)])
    check_all({"bn-relu y": to_nchw(outs[0]), "bn-relu dx": to_nchw(gin[0]), "bn-relu dgamma": gp[0]}, ref)
    # max-pool 3/2/1, avg-pool 4, add+relu, concat
    x = rnd(N, 64, 16, 16, seed=5)
    gy_max, gy_avg = rnd(N, 64, 8, 8, seed=6), rnd(N, 64, 4, 4, seed=7)
    a, b = rnd(N, 64, 8, 8, seed=8), rnd(N, 128, 8, 8, seed=9)
    gy = rnd(N, 192, 8, 8, seed=10)

    def ref(dt):
        out = {}
        xr = x.to(dt).requires_grad_()
        yr = F.max_pool2d(xr, 3, 2, 1)
        out.update(zip(("maxpool y", "maxpool dx"), [yr.detach()] + grads(yr, [xr], gy_max)))
        xr = x.to(dt).requires_grad_()
        yr = F.adaptive_avg_pool2d(xr, 4)
        out.update(zip(("avgpool y", "avgpool dx"), [yr.detach()] + grads(yr, [xr], gy_avg)))
        ar, brr = a.to(dt).requires_grad_(), b.to(dt).requires_grad_()
        yr = F.relu(torch.cat([ar, brr], 1) + 0.1)
        out.update(zip(("concat+add_relu y", "concat+add_relu da", "concat+add_relu db"),
                       [yr.detach()] + grads(yr, [ar, brr], gy)))
        return out
    got = {}
    outs, gin, _ = run_tape(lambda t, a_: T.maxpool3s2(t, a_), [to_pix(x).to(dev)], [], lambda o: [to_pix(gy_max).to(dev)])
    got.update({"maxpool y": to_nchw(outs[0]), "maxpool dx": to_nchw(gin[0])})
    outs, gin, _ = run_tape(lambda t, a_: T.avgpool(t, a_, 4), [to_pix(x).to(dev)], [], lambda o: [to_pix(gy_avg).to(dev)])
    got.update({"avgpool y": to_nchw(outs[0]), "avgpool dx": to_nchw(gin[0])})
    bias = torch.full((N, 8, 8, 192), 0.1, device=dev)
    outs, gin, _ = run_tape(lambda t, p, q: T.add_relu(t, T.concat_channels(t, [p, q]), bias),
                            [to_pix(a).to(dev), to_pix(b).to(dev)], [], lambda o: [to_pix(gy).to(dev)])
    got.update({"concat+add_relu y": to_nchw(outs[0]), "concat+add_relu da": to_nchw(gin[0]),
                "concat+add_relu db": to_nchw(gin[1])})
    check_all(got, ref)


@pytest.mark.gpu
def test_r18_vs_reference_golden_and_oracle(golden_dir):
    dev = _dev()
    from unidefense_amd.loss import LOSSES
    from unidefense_amd.model import load_model
    g = np.load(os.path.join(golden_dir, "udr18_n8.npz"))
    n, size, seed, mseed = [int(v) for v in g["meta"]]
    x = param_fill.make_input(n, size, seed)
    tgt = param_fill.make_labels(n)
    rng = make_rng_r18(n, mseed)
    m = load_model("UDR18")(num_classes=2, drop_rate=0.5)
    param_fill.fill_module_(m, sf_coef=0.0, fuse_coef=0.3)
    m = m.to(dev)
    with torch.no_grad():
        _check_outputs(m.eval()(x.to(dev)), g, "eval_", 1e-3)
    lam = ou.SMOOTH_LAMBDAS
    m.train()
    m._debug_watch = True
    out = m(x.to(dev), rng=rng)
    _check_outputs(out, g, "train_", 1e-3)
    # the 3x3 max-pool of emb_block1 has top-2 gaps down to ~1e-6 in every batch: pin the oracle's winners to
    # the HIP path's (the oracle asserts each pinned winner is a maximum within 1e-4 of max|z|) so that the gradients
    # are compared on the same branch; the float32 CPU run keeps its own arg-max and shows the effect of a flip
    sel = m._debug_feats["pool_sel"].permute(0, 3, 1, 2).cpu()
    # ... and likewise the on/off pattern of every ReLU (oracle/r18.py:relu_site checks that the pattern departs
    # from the oracle's own only on units within 1e-4 of zero): a ReLU network's gradient is piecewise constant in
    # those signs, ~10 of the ~1e7 units of this batch sit within fp32 rounding of 0, and each flip moves some
    # weight gradients by ~1e-2 — two correct fp32 evaluations that round differently land on different pieces
    masks = {k: v.permute(0, 3, 1, 2).cpu() for k, v in m._debug_kinks.items()}
    pinned = dict(rng, pool_sel=sel, relu_masks=masks)
    sd64 = r18_state(torch.float64, requires_grad=True)
    o64 = r18.forward_r18(sd64, x.double(), training=True, drop_rate=0.5, rng=pinned)
    sites = set(masks) - {"_used", "_departures"}
    assert masks["_used"] == sites, sorted(sites - masks["_used"])
    dep = masks["_departures"]
    print(f"  pinned {len(sites)} ReLU sites + the max-pool winners to the HIP path's pattern: "
          f"{dep['relu_flips']} of {dep['relu_units']} ReLU units and {dep['pool_moves']} of {dep['pool_windows']} "
          f"pool windows depart from the float64 evaluation's own choice (each checked to be a near-tie)")
    # the pinning may only ever touch a vanishing share of the decisions: a wrong-sign kernel would flip a large part
    assert dep["relu_flips"] <= 2e-5 * dep["relu_units"] + 20 and dep["pool_moves"] <= 2e-4 * dep["pool_windows"] + 20, dep
    _loss(o64, tgt, lam).backward()
    sd32 = r18_state(requires_grad=True)
    _loss(r18.forward_r18(sd32, x, training=True, drop_rate=0.5, rng=pinned), tgt, lam).backward()
    # Conditioning yardstick, independent of any implementation: how far the EXACT (float64) gradient moves, on the
    # same pinned piece, when the input is perturbed by one fp32 ulp (1e-7 relative).
    sens = {}
    for pseed in (1, 2):
        gp = torch.Generator().manual_seed(pseed)
        xp = x.double() * (1.0 + 1e-7 * torch.randn(x.shape, generator=gp, dtype=torch.float64))
        sdp = r18_state(torch.float64, requires_grad=True)
        _loss(r18.forward_r18(sdp, xp, training=True, drop_rate=0.5, rng=pinned), tgt, lam).backward()
        for k, v in sdp.items():
            if v.grad is not None:
                sens[k] = max(sens.get(k, 0.0), (v.grad - sd64[k].grad).abs().max().item())
    ld, t = out["loss_dict"], tgt.to(dev)
    trip = sum(LOSSES["aw_triplet"](f, t) for f in ld["triplet"])
    total = LOSSES["cross_entropy"](out["cls_out"], t) + lam["lambda_mask"] * (ld["freq_mask"].mean() + ld["spat_mask"].mean()) \
        + lam["lambda_triplet"] * trip
    e = abs(total.item() - float(g["smooth_loss_total_loss"])) / abs(float(g["smooth_loss_total_loss"]))
    assert within("smooth total loss", e, 1e-3), e
    total.backward()
    rows = []
    for k, p in m.named_parameters():
        if p.grad is None:
            continue
        ref = sd64[k].grad
        d = (p.grad.detach().double().cpu() - ref).abs().max().item()
        s = ref.abs().max().item()
        d32 = (sd32[k].grad.double() - ref).abs().max().item()
        # on the pinned piece the problem is smooth: 1e-4 of the tensor's scale (observed: <= 2e-5), never looser
        # than 5x what the CPU fp32 run or a one-ulp input perturbation do to the same gradient
        rows.append((d / max(1e-4 * s + 2e-6, 5.0 * d32, 5.0 * sens.get(k, 0.0)), k, d, s, d32, sens.get(k, 0.0)))
    rows.sort(reverse=True)
    for r in rows[:10]:
        print("  %.3f  %-50s maxerr %.3e  maxref %.3e  cpu-fp32-err %.3e  ulp-sensitivity %.3e" % r)
    within("worst gradient tensor: max err / max(floor, 5 x oracle fp32 err, 5 x one-ulp sensitivity)", rows[0][0], 1.0)
    bad = [r for r in rows if not r[0] < 1.0]
    assert not bad, bad[:10]


@pytest.mark.gpu
@pytest.mark.parametrize("name,size", [("UDR18", 128), ("UDR50", 256)])
def test_resnet_constructor_variant_eval_vs_reference_golden(golden_dir, name, size):
    """bias=True + affine=False on the embedder / decoder / filter convs and norms of the two ResNet models (model/unidefense.py:
    268-270, 448-450; resnet/module_exp.py:62-75: the SFConv's bias sits on its spatial branch) against eval outputs recorded
    from the reference built the same way (oracle/make_golden_variants.py res); state-dict keys as the reference's; and a
    train-mode backward runs through every bias (their gradients are finite and non-zero)."""
    dev = _dev()
    from unidefense_amd.model import load_model
    from oracle import r50
    g = np.load(os.path.join(golden_dir, f"{name.lower()}_eval_n2_bias_noaffine.npz"))
    n, sz, seed = [int(v) for v in g["meta"]]
    assert sz == size
    m = load_model(name)(num_classes=2, drop_rate=0.5, bias=True, affine=False)
    want = (r18.r18_state_shapes if name == "UDR18" else r50.r50_state_shapes)(2, bias=True, affine=False)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    param_fill.fill_module_(m, sf_coef=0.0, fuse_coef=0.3)
    m = m.to(dev)
    x = param_fill.make_input(n, size, seed).to(dev)
    with torch.no_grad():
        _check_outputs(m.eval()(x), g, "eval_", 1e-3)
    m.train()
    out = m(x)
    (out["cls_out"].sum() + out["rec"].mean() + out["loss_dict"]["freq_mask"].mean() + out["loss_dict"]["spat_mask"].mean()).backward()
    biases = [(k, p) for k, p in m.named_parameters() if k.endswith(".bias") and k.split(".")[0] in
              ("emb_block1", "emb_block2", "dec_block1", "dec_block2", "dec_block3", "freq_filter", "spat_filter")]
    assert len(biases) >= 16
    for k, p in biases:
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, k


@pytest.mark.gpu
@pytest.mark.parametrize("name,size", [("UDR50", 224), ("UDR18", 224)])
def test_resnet_models_at_sizes_without_an_in_register_fft(name, size):
    """224 x 224 (feature maps 56 / 28 / 14 / 7): no side has an in-register transform in csrc/fft.hip, every SFConv goes through
    DFT matrices on the GEMM kernels (kernels._rfft2_generic / _irfft2_generic) — eval outputs against the oracle, and a train
    step runs with finite gradients for every parameter that takes one"""
    dev = _dev()
    from unidefense_amd.model import load_model
    from oracle import r50
    shapes, fwd = (r18.r18_state_shapes, r18.forward_r18) if name == "UDR18" else (r50.r50_state_shapes, r50.forward_r50)
    m = load_model(name)(num_classes=2, drop_rate=0.5)
    param_fill.fill_module_(m, sf_coef=0.0, fuse_coef=0.3)
    m = m.to(dev)
    x = param_fill.make_input(2, size, seed=5)
    sd = param_fill.fill_state_dict(shapes(2), 0.0, 0.3)
    with torch.no_grad():
        ref = fwd(sd, x, training=False)
        got = m.eval()(x.to(dev))
    for k in ("cls_out", "rec"):
        assert within(f"{name} at {size}: eval {k} vs oracle", _rel(got[k], ref[k]), 1e-3)
    for k in ("freq_mask", "spat_mask", "spatial", "freq"):
        assert within(f"{name} at {size}: eval {k} vs oracle", _rel(got["loss_dict"][k], ref["loss_dict"][k]), 1e-3)
    m.train()
    out = m(x.to(dev))
    (out["cls_out"].sum() + out["rec"].mean() + out["loss_dict"]["freq"].mean()).backward()
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert len(grads) >= 100 and all(torch.isfinite(g_).all() for g_ in grads)
