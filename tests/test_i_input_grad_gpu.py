"""Gradients with respect to the input image (x.grad of model(x)) on the MI355X: the stem data-gradient kernel against
torch in float64, x.grad of UDEB4 / UDR18 / UDR50 against the float64 oracles' autograd, the frozen-model backward (no
weight-gradient work), graph capture, and the paths that must stay as they were when x does not require grad."""
import pytest
import torch
import torch.nn.functional as F

from oracle import eb4, losses as OL, param_fill, r18, r50
from tests import oracle_util as ou
from tests.margins import within

pytestmark = pytest.mark.gpu

GRAD_BAR = 1e-3          # the suite's plain gradient bound: max|d| / max|ref| and relative L2


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _udeb4(dev):
    from unidefense_amd.model import load_model
    m = load_model("UDEB4")(extractor="efficientnet-b4", num_classes=2, drop_rate=0.5)
    param_fill.fill_module_(m, sf_coef=0.0, fuse_coef=0.3)
    return m.to(dev)


def _resnet(name, dev):
    from unidefense_amd.model import load_model
    m = load_model(name)(num_classes=2, drop_rate=0.5)
    param_fill.fill_module_(m, sf_coef=0.0, fuse_coef=0.3)
    return m.to(dev)


def _freeze(m, frozen):
    for p in m.parameters():
        p.requires_grad_(not frozen and p is not getattr(m.bottleneck, "bias", None))
    return m


def _errs(g, ref):
    g, ref = g.detach().double().cpu(), ref.detach().double().cpu()
    d = g - ref
    return float(d.abs().max() / ref.abs().max()), float(d.norm() / ref.norm())


def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def _smooth(o):
    """the smooth scalar of tests/test_c_model_gpu.py::test_eval_mode_backward_vs_oracle"""
    ld = o["loss_dict"]
    return (o["cls_out"] * o["cls_out"]).sum() + 10.0 * (o["rec"] * o["rec"]).mean() + ld["freq_mask"].mean() \
        + ld["spat_mask"].mean() + sum((f * f).mean() for f in ld["triplet"])


def _ce(tgt):
    return lambda o: F.cross_entropy(o["cls_out"], tgt.to(o["cls_out"].device))


# ---------------------------------------------------------------------------------------------------------------- kernel
_STEMS = [(3, 48, 0, 1, s) for s in (256, 380, 224)] + [(7, 64, 3, 3, s) for s in (128, 160, 224, 256, 320)]


@pytest.mark.parametrize("k,co,pad_t,pad_b,size", _STEMS)
def test_stem_dgrad_vs_float64(k, co, pad_t, pad_b, size):
    """ud_stem_dgrad against torch.nn.grad.conv2d_input in float64: every element within 2e-6 of sum |w dy| over its terms
    (the GEMM accuracy rule), with accumulate off and on."""
    from unidefense_amd import kernels as K
    dev = _dev()
    gen = torch.Generator().manual_seed(size * 10 + k)
    for n, accumulate in ((1, False), (3, True), (32 if size == 256 else 2, size % 2 == 0)):
        Ho = (size + pad_t + pad_b - k) // 2 + 1
        dy = torch.randn(n, Ho, Ho, co, generator=gen)
        w = torch.randn(co, 3, k, k, generator=gen) * 0.2
        base = torch.randn(n, 3, size, size, generator=gen) if accumulate else None
        g = K.conv_geom(n, size, size, 3, Ho, Ho, k, k, 2, pad_t, pad_t, 0)
        out = base.to(dev).contiguous() if accumulate else None
        got = K.stem_dgrad(dy.to(dev), w.to(dev), g, out=out)
        if accumulate:
            assert got.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()

        def ref_of(d, ww):
            # F.conv2d with pads (pad_t before, pad_b after): pad the input, so the gradient is the padded one cropped
            full = torch.nn.grad.conv2d_input((n, 3, size + pad_t + pad_b, size + pad_t + pad_b), ww, d.permute(0, 3, 1, 2),
                                              stride=2)
            return full[:, :, pad_t:pad_t + size, pad_t:pad_t + size]
        ref = ref_of(dy.double(), w.double())
        mag = ref_of(dy.double().abs(), w.double().abs())
        if accumulate:
            ref = ref + base.double()
            mag = mag + base.double().abs()
        err = (got.double().cpu() - ref).abs()
        worst = float((err / (mag + 1e-30)).max())
        assert (err <= 2e-6 * mag + 1e-12).all(), (k, size, n, accumulate, worst)


# ---------------------------------------------------------------------------------------------------------------- UDEB4
def test_udeb4_eval_input_grad_vs_oracle():
    """x.grad of an eval-mode UDEB4 (n=1, 256^2) against the float64 oracle for the smooth scalar and for cross-entropy on
    cls_out, with parameters requiring grad and with a frozen model; the frozen backward gives no parameter a .grad and the
    same x.grad as the unfrozen one up to summation order."""
    dev = _dev()
    m = _udeb4(dev).eval()
    x = param_fill.make_input(1, 256, 7)
    tgt = param_fill.make_labels(1)
    sd = ou.oracle_state(0.0, 0.3, dtype=torch.float64)
    x64 = x.double().requires_grad_()
    ref = eb4.forward_eb4(sd, x64, training=False)
    objectives = {"smooth": _smooth, "cross_entropy": _ce(tgt)}
    refs = {}
    for name, f in objectives.items():
        refs[name], = torch.autograd.grad(f(ref), x64, retain_graph=True)
    for name, f in objectives.items():
        got = {}
        for frozen in (False, True):
            _freeze(m, frozen)
            m.zero_grad(set_to_none=True)
            xg = x.to(dev).requires_grad_()
            f(m(xg)).backward()
            torch.cuda.synchronize()
            assert xg.grad is not None and torch.isfinite(xg.grad).all()
            if frozen:
                assert all(p.grad is None for p in m.parameters())
            else:
                assert m.classifier.fc.weight.grad is not None
            mx, l2 = _errs(xg.grad, refs[name])
            print(f"  {name} frozen={frozen}: max|d|/max|ref| {mx:.2e}  rel L2 {l2:.2e}")
            assert within(f"UDEB4 eval x.grad ({name}, frozen={frozen}), max|d| / max|ref|", mx, GRAD_BAR)
            assert within(f"UDEB4 eval x.grad ({name}, frozen={frozen}), rel L2", l2, GRAD_BAR)
            got[frozen] = xg.grad.clone()
        d = _rel_l2(got[True], got[False])
        assert within(f"UDEB4 eval x.grad ({name}): frozen vs unfrozen rel L2", d, 1e-5)
    _freeze(m, False)


def _train_x_grad(m, x, tgt, rng, dev, lam, loss_scale=1.0):
    m.train()
    m._dec_dropout = True
    xg = x.to(dev).requires_grad_()
    out = m(xg, rng=rng)
    n = len(tgt)
    (OL.pass1_loss(out, tgt.to(dev), n // 2, n - n // 2, lam)["total_loss"] * loss_scale).backward()
    torch.cuda.synchronize()
    return xg.grad / loss_scale


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "operator"])
def test_udeb4_train_input_grad_vs_oracle(fused):
    """x.grad of a UDEB4 training forward (n=4, 256^2, pinned drop masks, no perturbation) under the pass-1 loss against the
    float64 oracle, on the fused MBConv path and on the operator path."""
    from unidefense_amd.config import override
    dev = _dev()
    n = 4
    x = param_fill.make_input(n, 256, 21)
    tgt = param_fill.make_labels(n)
    rng = ou.make_rng(n, 22, 0.5)
    sd = ou.oracle_state(0.0, 0.3, dtype=torch.float64)
    x64 = x.double().requires_grad_()
    out64 = eb4.forward_eb4(sd, x64, training=True, drop_rate=0.5, rng=rng)
    OL.pass1_loss(out64, tgt, n // 2, n - n // 2, ou.LAMBDAS)["total_loss"].backward()
    m = _udeb4(dev)
    with override(fused_mbconv=fused):
        g = _train_x_grad(m, x, tgt, rng, dev, ou.LAMBDAS)
    assert g is not None and torch.isfinite(g).all()
    mx, l2 = _errs(g, x64.grad)
    print(f"  fused={fused}: max|d|/max|ref| {mx:.2e}  rel L2 {l2:.2e}")
    assert within(f"UDEB4 train x.grad (fused={fused}), max|d| / max|ref|", mx, GRAD_BAR)
    assert within(f"UDEB4 train x.grad (fused={fused}), rel L2", l2, GRAD_BAR)


def test_udeb4_half_storage_train_input_grad():
    """Half-storage training (fp16 MBConv trunk, loss scale 2^10): x.grad is finite, and its relative L2 distance to the fp32
    x.grad stays within 4 x what ONE fp16 rounding of the parameters and the input does to the fp32 x.grad (the yardstick of
    tests/test_e_mixed_precision_gpu.py).  The proposed flat bar of 5e-2 is recorded, not asserted: x.grad is a per-pixel
    gradient through the whole trunk, with no sum over pixels to average the fp16 rounding out."""
    dev = _dev()
    n = 4
    x = param_fill.make_input(n, 256, 21)
    tgt = param_fill.make_labels(n)
    rng = ou.make_rng(n, 22, 0.5)
    m = _udeb4(dev)
    g32 = _train_x_grad(m, x, tgt, rng, dev, ou.LAMBDAS, 1024.0).clone()
    w32 = m.backbone._conv_stem.weight.grad.clone()
    m.zero_grad(set_to_none=True)
    m.half_storage = True
    try:
        g16 = _train_x_grad(m, x, tgt, rng, dev, ou.LAMBDAS, 1024.0)
        w16 = m.backbone._conv_stem.weight.grad.clone()
    finally:
        m.half_storage = False
    assert torch.isfinite(g16).all()
    # the yardstick: the fp32 step on parameters and input rounded once to fp16
    my = _udeb4(dev)
    with torch.no_grad():
        for p in my.parameters():
            p.copy_(p.half().float())
    gy = _train_x_grad(my, x.half().float(), tgt, rng, dev, ou.LAMBDAS, 1024.0)
    wy = my.backbone._conv_stem.weight.grad
    d, y = _rel_l2(g16, g32), _rel_l2(gy, g32)
    print(f"  x.grad rel L2 to fp32: half storage {d:.3e}, one fp16 rounding {y:.3e}; stem weight gradient: "
          f"{_rel_l2(w16, w32):.3e} / {_rel_l2(wy, w32):.3e}")
    within("UDEB4 half-storage train x.grad vs fp32, rel L2 (proposed 5e-2, recorded)", d, 5e-2)
    assert within("UDEB4 half-storage train x.grad vs fp32: deviation / (4 x one-rounding yardstick)", d / (4.0 * y), 1.0)


# ---------------------------------------------------------------------------------------------------------------- ResNets
@pytest.mark.parametrize("name,size", [("UDR18", 128), ("UDR50", 256)])
def test_resnet_eval_input_grad_vs_oracle(name, size):
    """x.grad of the eval-mode ResNet models (n=2) against the float64 oracle, the ReLU patterns and max-pool winners pinned
    to the HIP path's (tape.kinks), as the ResNet gradient tests do."""
    dev = _dev()
    n = 2
    x = param_fill.make_input(n, size, 5)
    tgt = param_fill.make_labels(n)
    m = _resnet(name, dev).eval()
    m._debug_watch = True
    try:
        xg = x.to(dev).requires_grad_()
        out = m(xg)
        kinks = {k: v.permute(0, 3, 1, 2).cpu() for k, v in m._debug_kinks.items()}
        feats = m._debug_feats
        (_smooth(out) + _ce(tgt)(out)).backward()
        torch.cuda.synchronize()
    finally:
        m._debug_watch = False
    if name == "UDR18":
        sel = feats["pool_sel"].permute(0, 3, 1, 2).cpu()
        sd = param_fill.fill_state_dict(r18.r18_state_shapes(2), 0.0, 0.3, torch.float64)
        fwd = r18.forward_r18
    else:
        sel = {"stem": feats["pool_sel_stem"].permute(0, 3, 1, 2).cpu(), "emb": feats["pool_sel_emb"].permute(0, 3, 1, 2).cpu()}
        sd = param_fill.fill_state_dict(r50.r50_state_shapes(2), 0.0, 0.3, torch.float64)
        fwd = r50.forward_r50
    x64 = x.double().requires_grad_()
    o64 = fwd(sd, x64, training=False, rng={"pool_sel": sel, "relu_masks": kinks})
    (_smooth(o64) + _ce(tgt)(o64)).backward()
    mx, l2 = _errs(xg.grad, x64.grad)
    print(f"  {name} {size}: max|d|/max|ref| {mx:.2e}  rel L2 {l2:.2e}")
    assert within(f"{name} eval x.grad, max|d| / max|ref|", mx, GRAD_BAR)
    assert within(f"{name} eval x.grad, rel L2", l2, GRAD_BAR)


# ---------------------------------------------------------------------------------------------------------------- contract
def test_param_grads_unchanged_by_input_tracking():
    """The same training forward and objective with and without x.requires_grad give bitwise-equal parameter gradients
    (the suite's deterministic configuration), on the fused path and in eval mode."""
    dev = _dev()
    n = 2
    x = param_fill.make_input(n, 256, 31)
    tgt = param_fill.make_labels(n)
    m = _udeb4(dev)
    for mode in ("train", "eval"):
        res = []
        for track in (False, True):
            m.train(mode == "train")
            m.zero_grad(set_to_none=True)
            xi = x.to(dev).requires_grad_(track)
            out = m(xi, rng=ou.make_rng(n, 32, 0.5))
            OL.pass1_loss(out, tgt.to(dev), n // 2, n - n // 2, ou.LAMBDAS)["total_loss"].backward()
            torch.cuda.synchronize()
            assert (xi.grad is not None) == track
            res.append({k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
        assert res[0].keys() == res[1].keys() and len(res[0]) > 400
        diff = [k for k in res[0] if not torch.equal(res[0][k], res[1][k])]
        assert not diff, (mode, diff[:10])


def test_untracked_forward_never_reaches_input_grad_kernels(monkeypatch):
    """Additivity: with x not requiring grad, the training (fused and operator paths) and eval forwards + backwards never call
    the new wrappers or the tape's x-path nodes."""
    from unidefense_amd import kernels as K, tape as T
    from unidefense_amd.config import override

    def boom(*a, **k):
        raise AssertionError("input-gradient code reached with x.requires_grad = False")
    for mod, name in ((K, "stem_dgrad"), (K, "absdiff_bwd"), (K, "outer"), (T, "planes_to_pix"), (T, "absdiff"),
                      (T, "_stem_dgrad")):
        monkeypatch.setattr(mod, name, boom)
    dev = _dev()
    n = 2
    x = param_fill.make_input(n, 256, 41).to(dev)
    tgt = param_fill.make_labels(n).to(dev)
    m = _udeb4(dev)
    for fused in (True, False):
        with override(fused_mbconv=fused):
            m.train()
            out = m(x, rng=ou.make_rng(n, 42, 0.5))
            OL.pass1_loss(out, tgt, n // 2, n - n // 2, ou.LAMBDAS)["total_loss"].backward()
    m.eval()
    _smooth(m(x)).backward()
    with torch.no_grad():
        m(x)
    torch.cuda.synchronize()


def test_frozen_input_grad_graph_capture():
    """A frozen eval model: one eager call, then forward + backward to x captured into a hipGraph; replays are bitwise equal
    to each other and within 1e-5 relative L2 of the eager x.grad."""
    dev = _dev()
    m = _freeze(_udeb4(dev).eval(), True)
    x = param_fill.make_input(2, 256, 51).to(dev)
    xs = x.clone().requires_grad_()

    def step():
        g, = torch.autograd.grad(_smooth(m(xs)), xs)
        return g
    eager = step().clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gx = step()
    reps = []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        reps.append(gx.clone())
    assert torch.isfinite(reps[0]).all()
    assert all(torch.equal(r, reps[0]) for r in reps[1:])
    d = _rel_l2(reps[0], eager)
    assert within("captured frozen x.grad vs eager, rel L2", d, 1e-5)
    del graph


def test_perturbed_training_forward_leaves_x_grad_none():
    """A perturbed training forward (pert lists) passes no gradient back to x, as documented."""
    dev = _dev()
    n = 2
    m = _udeb4(dev).train()
    x = param_fill.make_input(n, 256, 61).to(dev).requires_grad_()
    tgt = param_fill.make_labels(n).to(dev)
    torch.manual_seed(63)
    idx = torch.tensor([0])            # one real and one fake sample: each half's perturbation source is itself
    out = m(x, pert_real_list=idx, pert_fake_list=idx, preserve_color=True, rng=ou.make_rng(n, 62, 0.5))
    OL.pass1_loss(out, tgt, n // 2, n - n // 2, ou.LAMBDAS)["total_loss"].backward()
    torch.cuda.synchronize()
    assert x.grad is None
    assert m.classifier.fc.weight.grad is not None


def test_frozen_input_grad_under_data_parallel():
    """HipDataParallel in a world of one rank with cfg.force_collectives (the gradient reducer on the model): a frozen x.grad
    pass before and after training backwards leaves the reducer and its learned use counts alone — it gives the plain frozen
    model's x.grad bit for bit, and the training backwards around it keep working."""
    import os
    import torch.distributed as dist
    from unidefense_amd.config import override
    from unidefense_amd.engine.parallel import HipDataParallel
    dev = _dev()
    torch.cuda.set_device(dev)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29577")
    n = 2
    x = param_fill.make_input(n, 256, 81).to(dev)
    tgt = param_fill.make_labels(n).to(dev)

    plain = _freeze(_udeb4(dev).eval(), True)
    xg = x.clone().requires_grad_()
    _smooth(plain(xg)).backward()
    ref = xg.grad.clone()
    del plain

    def frozen_pass(m, dp):
        m.eval()
        _freeze(m, True)
        m.zero_grad(set_to_none=True)
        xf = x.clone().requires_grad_()
        _smooth(dp(xf)).backward()
        torch.cuda.synchronize()
        assert all(p.grad is None for p in m.parameters())
        _freeze(m, False)
        return xf.grad

    def train_pass(m, dp):
        bufs = {k: v.clone() for k, v in m.named_buffers()}
        m.train()
        m.zero_grad(set_to_none=True)
        out = dp(x, rng=ou.make_rng(n, 82, 0.5))
        OL.pass1_loss(out, tgt, n // 2, n - n // 2, ou.LAMBDAS)["total_loss"].backward()
        torch.cuda.synchronize()
        assert m.classifier.fc.weight.grad is not None
        with torch.no_grad():              # the training forward moved the BatchNorm running statistics: put them back, so
            for k, v in m.named_buffers():  # that the eval passes around it see the same model as the plain reference
                v.copy_(bufs[k])

    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        with override(force_collectives=True):
            m = _udeb4(dev)
            dp = HipDataParallel(m, sync_bn=False)
            assert getattr(m, "_grad_reducer", None) is not None
            assert torch.equal(frozen_pass(m, dp), ref)           # first: nothing learned yet
            assert getattr(m, "_param_uses", None) is None
            train_pass(m, dp)                                     # learns the use counts
            uses = dict(m._param_uses)
            assert torch.equal(frozen_pass(m, dp), ref)           # after a training backward
            assert m._param_uses == uses
            train_pass(m, dp)                                     # compares them: unchanged
    finally:
        if created:
            dist.destroy_process_group()
