"""GPU: the graph-captured inference forward (unidefense_amd/infer.py: InferenceRunner), the eval-mode MBConv node with the
expand conv inside the depthwise pass (csrc/evalblk.hip: ud_mb_eval_dw) and the eval form of ud_bn_ref (sum = NULL: the
running statistics, read in place).

Bars: model outputs as tests/test_c_model_gpu.py (1e-3 of each tensor's max magnitude against the reference goldens and the
float64 oracle); the kernel against float64 torch formulas within 2e-6 of the same chain evaluated on absolute values (the
GEMMs' bound of sum |a||b|, carried through BN and swish).
"""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import eb4, param_fill
from tests import oracle_util as ou
from tests.margins import within
from tests.test_c_model_gpu import RTOL, _check_outputs, _close, _model, _variant_model

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _flat(out):
    ld = out["loss_dict"]
    d = {"cls_out": out["cls_out"], "rec": out["rec"]}
    for k in ("factorization", "freq_mask", "spat_mask", "spatial", "freq"):
        d[k] = ld[k]
    for i, t in enumerate(ld["triplet"]):
        d[f"triplet{i}"] = t
    return d


def _replayed(m, x):
    """the runner's second call: the captured graph's replay (the first is the eager warm-up)"""
    from unidefense_amd.infer import InferenceRunner
    r = InferenceRunner(m, x.shape[0], x.shape[-1])
    r(x)
    out = r(x)
    assert r.graph is not None
    return r, out


# ---- 1. reference eval goldens through the runner --------------------------------------------------------------------------
@pytest.mark.parametrize("fname,sf,fuse", [("udeb4_eval_n2.npz", 0.0, 0.3), ("udeb4_eval_n2_init.npz", -10.0, 0.0),
                                           ("udeb4_eval_n2_s380.npz", 0.0, 0.3)])
def test_runner_vs_reference_eval_golden(golden_dir, fname, sf, fuse):
    dev = _dev()
    g = np.load(os.path.join(golden_dir, fname))
    n, size, seed = [int(v) for v in g["meta"]]
    m = _model(dev, sf, fuse).eval()
    _, out = _replayed(m, param_fill.make_input(n, size, seed).to(dev))
    _check_outputs(out, g)


@pytest.mark.parametrize("tag,bias,affine", [("bias_noaffine", True, False), ("bias", True, True), ("noaffine", False, False)])
def test_runner_constructor_variants_vs_reference_golden(golden_dir, tag, bias, affine):
    dev = _dev()
    g = np.load(os.path.join(golden_dir, f"udeb4_eval_n2_{tag}.npz"))
    n, size, seed = [int(v) for v in g["meta"]]
    m = _variant_model(dev, bias, affine).eval()
    _, out = _replayed(m, param_fill.make_input(n, size, seed).to(dev))
    _check_outputs(out, g)


# ---- 2. float64 oracle and the eager eval forward ---------------------------------------------------------------------------
def test_runner_vs_oracle_n4():
    dev = _dev()
    x = param_fill.make_input(4, 256, 21)
    sd = ou.oracle_state(0.0, 0.3)
    with torch.no_grad():
        ref = _flat(eb4.forward_eb4(sd, x, training=False))
    m = _model(dev, 0.0, 0.3).eval()
    _, out = _replayed(m, x.to(dev))
    got = _flat(out)
    bad = [(k, e) for k, e in (_close(got[k], ref[k], k) for k in ref) if not within("runner vs oracle " + k, e, RTOL)]
    assert not bad, bad


@pytest.mark.parametrize("n,size", [(32, 256), (8, 380)])
def test_runner_vs_eager_eval(n, size):
    dev = _dev()
    m = _model(dev, 0.0, 0.3).eval()
    x = param_fill.make_input(n, size, 31).to(dev)
    with torch.no_grad():
        ref = {k: v.clone() for k, v in _flat(m(x)).items()}
    _, out = _replayed(m, x)
    got = _flat(out)
    bad = [(k, e) for k, e in ((k, _rel(got[k], ref[k])) for k in ref) if not within(f"runner vs eager {k}", e, RTOL)]
    assert not bad, bad


# ---- 3. sample independence -------------------------------------------------------------------------------------------------
def test_runner_samples_independent_bs96():
    dev = _dev()
    from unidefense_amd.infer import InferenceRunner
    m = _model(dev, 0.0, 0.3).eval()
    x = param_fill.make_input(96, 256, 41).to(dev)
    _, big = _replayed(m, x)
    cls, rec = big["cls_out"].clone(), big["rec"].clone()
    one = InferenceRunner(m, 1, 256)
    wc = wr = 0.0
    for i in range(96):
        o = one(x[i:i + 1].contiguous())
        wc, wr = max(wc, _rel(o["cls_out"], cls[i:i + 1])), max(wr, _rel(o["rec"], rec[i:i + 1]))
    assert one.graph is not None
    # cls_out to 1e-5; rec to 1e-4: the large 1x1 convs split each operand into fp16 planes with ONE power-of-two scale per
    # tensor, so the rounding of an image's operands depends on the batch's largest value, and the decoder's
    # InstanceNorms amplify that rounding in the reconstruction (observed 2.9e-5 at bs 96 against bs 1)
    assert within("bs-96 replay vs bs-1 runner, cls_out, worst image", wc, 1e-5)
    assert within("bs-96 replay vs bs-1 runner, rec, worst image", wr, 1e-4)


# ---- 4. replays, and a runner that follows the model ------------------------------------------------------------------------
def test_replay_bitwise_and_follows_optimizer_step():
    dev = _dev()
    m = _model(dev, 0.0, 0.3).eval()
    x = param_fill.make_input(4, 256, 51).to(dev)
    r, out = _replayed(m, x)
    a = {k: v.clone() for k, v in _flat(out).items()}
    b = _flat(r(x))
    assert all(torch.equal(a[k], b[k]) for k in a)
    # in-place AdamW step on every parameter and new running statistics of one BatchNorm
    torch.manual_seed(5)
    params = [p for p in m.parameters() if p.requires_grad]
    for p in params:
        p.grad = torch.randn_like(p) * 1e-2
    opt = torch.optim.AdamW(params, lr=1e-3)
    ptrs = [p.data_ptr() for p in params]
    opt.step()
    assert ptrs == [p.data_ptr() for p in params]
    bn = m.backbone._blocks[3]._bn0                       # a block of the eval-mode node (group 1)
    bn.running_mean.add_(0.05)
    bn.running_var.mul_(1.5)
    after = {k: v.clone() for k, v in _flat(r(x)).items()}
    with torch.no_grad():
        ref = _flat(m(x))
    moved = _rel(ref["cls_out"], a["cls_out"])
    assert moved > 1e-2, moved                            # the step changed the function
    bad = [(k, e) for k, e in ((k, _rel(after[k], ref[k])) for k in ref) if not within(f"same runner after the step {k}", e, RTOL)]
    assert not bad, bad


# ---- 5. the kernel and the eval form of ud_bn_ref ---------------------------------------------------------------------------
def _eval_shapes():
    from unidefense_amd import kernels as K
    from unidefense_amd.model.arch import build_arch
    shapes = set()
    for size in (256, 320, 380):
        arch = build_arch("efficientnet-b4", "ortho", size)
        s = math.ceil(size / 2)
        for sp in arch["blocks"]:
            if sp.expand != 1 and sp.sf_norm is None and K.mb_eval_dw_ok(sp.cin, sp.cexp, sp.k, sp.stride):
                shapes.add((s, sp.cin, sp.cexp, sp.k, sp.stride, sp.pad))
            s = math.ceil(s / sp.stride)
    return sorted(shapes)


def _bn_mod(C, dev, seed):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm2d(C, eps=1e-3)
    with torch.no_grad():
        bn.weight.copy_(1 + 0.2 * torch.randn(C, generator=g))
        bn.bias.copy_(0.2 * torch.randn(C, generator=g))
        bn.running_mean.copy_(0.3 * torch.randn(C, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(C, generator=g))
    return bn.to(dev).eval()


def _bn64(z, bn):
    ga, be = bn.weight.double().cpu(), bn.bias.double().cpu()
    mu, var = bn.running_mean.double().cpu(), bn.running_var.double().cpu()
    sc = ga / torch.sqrt(var + bn.eps)
    return (z - mu.view(1, -1, 1, 1)) * sc.view(1, -1, 1, 1) + be.view(1, -1, 1, 1), sc.abs().view(1, -1, 1, 1)


def test_mb_eval_dw_shapes_cover_both_groups():
    sh = _eval_shapes()
    assert {s[4] for s in sh} == {1, 2} and {s[1] for s in sh} >= {24, 32, 272, 448}, sh


@pytest.mark.parametrize("shape", _eval_shapes() if torch.cuda.is_available() else [], ids=str)
def test_mb_eval_dw_vs_float64(shape):
    """d (both out_act forms) and the pooled SE squeeze against conv1x1 -> BN -> swish -> SAME-padded depthwise -> BN -> swish in
    float64, within 2e-6 of the same chain on absolute values; the running buffers are not written."""
    dev = _dev()
    from unidefense_amd import kernels as K
    H, Ci, CE, k, s, pad = shape
    N = 2
    g = torch.Generator().manual_seed(H * 7 + Ci + s)
    x = torch.randn(N, H, H, Ci, generator=g)
    we = torch.randn(CE, Ci, generator=g) / math.sqrt(Ci)
    w = torch.randn(CE, 1, k, k, generator=g) / k
    bn0, bn1 = _bn_mod(CE, dev, 1), _bn_mod(CE, dev, 2)
    keep = [t.clone() for t in (bn0.running_mean, bn0.running_var, bn1.running_mean, bn1.running_var)]
    pl, pr, pt, pb = pad
    Ho, Wo = (H + pt + pb - k) // s + 1, (H + pl + pr - k) // s + 1
    xd, wed, wtd = x.to(dev), we.to(dev), w.view(CE, k * k).t().contiguous().to(dev)
    d1, pool = K.mb_eval_dw(xd.contiguous(), wed, K.EvalBN(bn0, 1), wtd, K.EvalBN(bn1, 1), k, s, pt, pl, Ho, Wo, out_act=True)
    d0, pool0 = K.mb_eval_dw(xd.contiguous(), wed, K.EvalBN(bn0, 1), wtd, K.EvalBN(bn1, 1), k, s, pt, pl, Ho, Wo, out_act=False)
    torch.cuda.synchronize()
    for a, b in zip(keep, (bn0.running_mean, bn0.running_var, bn1.running_mean, bn1.running_var)):
        assert torch.equal(a, b)
    assert torch.equal(pool, pool0)
    # float64 chain and its bound
    x64 = x.double().permute(0, 3, 1, 2)
    e_lin = F.conv2d(x64, we.double().view(CE, Ci, 1, 1))
    e_abs = F.conv2d(x64.abs(), we.double().abs().view(CE, Ci, 1, 1))
    z0, sc0 = _bn64(e_lin, bn0)
    e = z0 * torch.sigmoid(z0)
    be = e_abs * sc0 * 1.1 + e.abs()                       # |swish'| <= 1.1
    dw = F.conv2d(F.pad(e, (pl, pr, pt, pb)), w.double(), stride=s, groups=CE)
    dw_abs = F.conv2d(F.pad(be, (pl, pr, pt, pb)), w.double().abs(), stride=s, groups=CE)
    z1, sc1 = _bn64(dw, bn1)
    d = z1 * torch.sigmoid(z1)
    bd = dw_abs * sc1 * 1.1 + d.abs()
    got0, got1 = d0.double().cpu().permute(0, 3, 1, 2), d1.double().cpu().permute(0, 3, 1, 2)
    r0 = float(((got0 - dw).abs() / dw_abs.clamp_min(1e-30)).max())
    r1 = float(((got1 - d).abs() / bd.clamp_min(1e-30)).max())
    rp = float(((pool.double().cpu() - d.mean((2, 3))).abs() / bd.mean((2, 3))).max())
    print(f"  {shape}: dw {r0:.2e}  d {r1:.2e}  pool {rp:.2e}")
    assert within(f"ud_mb_eval_dw raw {shape}", r0, 2e-6)
    assert within(f"ud_mb_eval_dw act {shape}", r1, 2e-6)
    assert within(f"ud_mb_eval_dw pool {shape}", rp, 2e-6)


def test_eval_form_bn_apply_and_colsum():
    dev = _dev()
    from unidefense_amd import kernels as K
    C, N, HW = 64, 3, 50
    bn = _bn_mod(C, dev, 3)
    keep = (bn.running_mean.clone(), bn.running_var.clone())
    x = torch.randn(N * HW, C, generator=torch.Generator().manual_seed(4)).to(dev)
    for act in (0, 1):
        y = K.bn_apply(x, K.EvalBN(bn, act), 1, N * HW)
        ref = F.batch_norm(x.double().cpu(), bn.running_mean.double().cpu(), bn.running_var.double().cpu(), bn.weight.double().cpu(),
                           bn.bias.double().cpu(), training=False, eps=bn.eps)
        if act:
            ref = ref * torch.sigmoid(ref)
        assert _rel(y, ref) < 1e-5, act
        acc = torch.zeros(N, C, dtype=torch.float64, device=dev)
        K.colsum_bn(x.view(N, HW, C).contiguous(), K.EvalBN(bn, act), N, HW, acc)
        assert _rel(acc, ref.view(N, HW, C).sum(1)) < 1e-5, act
    torch.cuda.synchronize()
    assert torch.equal(keep[0], bn.running_mean) and torch.equal(keep[1], bn.running_var)


def test_backward_entry_points_refuse_the_eval_form():
    dev = _dev()
    from unidefense_amd import kernels as K, lib
    C, R = 64, 64
    bn = _bn_mod(C, dev, 5)
    x, dy = torch.randn(R, C, device=dev), torch.randn(R, C, device=dev)
    out = torch.zeros(2 * C, dtype=torch.float64, device=dev)
    ref = ctypes.byref(K.EvalBN(bn, 1).ref())
    h = lib.load()
    assert h.ud_coldot_bn(K._p(dy), K._p(x), ref, 1, R, C, K._pd(out), None, 0, K._stream()) == -1000
    assert h.ud_normbwd_sums(K._p(x), K._p(dy), None, 1.0, ref, 0, 1, R, C, K._pd(out), K._pd(out, C), None, None, 0,
                             K._stream()) == -1000
    torch.cuda.synchronize()


# ---- 6. refusals and the ResNet variants ------------------------------------------------------------------------------------
def test_runner_refusals():
    dev = _dev()
    from unidefense_amd.infer import InferenceRunner
    m = _model(dev, 0.0, 0.3)
    with pytest.raises(ValueError, match="eval"):
        InferenceRunner(m.train(), 2, 256)
    r = m.eval().inference_runner(2, 256)
    assert m.inference_runner(2, 256) is r
    with pytest.raises(ValueError, match="cuda"):
        r(torch.zeros(2, 3, 256, 256))
    with pytest.raises(ValueError, match="differs"):
        r(torch.zeros(3, 3, 256, 256, device=dev))
    with pytest.raises(ValueError, match="differs"):
        r(torch.zeros(2, 3, 256, 256, device=dev, dtype=torch.float16))
    m.train()
    with pytest.raises(ValueError, match="training"):
        r(torch.zeros(2, 3, 256, 256, device=dev))
    assert r.calls == 0


@pytest.mark.parametrize("name,size", [("UDR18", 128), ("UDR50", 256)])
def test_resnet_runner_vs_reference_golden(golden_dir, name, size):
    dev = _dev()
    from tests.test_c_r18 import _check_outputs as check_res
    from unidefense_amd.model import load_model
    g = np.load(os.path.join(golden_dir, f"{name.lower()}_eval_n2_bias_noaffine.npz"))
    n, sz, seed = [int(v) for v in g["meta"]]
    assert sz == size
    m = load_model(name)(num_classes=2, drop_rate=0.5, bias=True, affine=False)
    param_fill.fill_module_(m, sf_coef=0.0, fuse_coef=0.3)
    m = m.to(dev).eval()
    _, out = _replayed(m, param_fill.make_input(n, size, seed).to(dev))
    check_res(out, g, "eval_", 1e-3)


# ---- 7. the engine hook -----------------------------------------------------------------------------------------------------
def test_engine_test_with_inference_graph():
    _dev()
    import copy
    from tests.test_d_train_engine import CONFIG
    from unidefense_amd.engine import get_engine
    res = []
    for graphed in (False, True):
        torch.manual_seed(0)
        cfg = copy.deepcopy(CONFIG)
        cfg["config"]["inference_graph"] = graphed
        eng = get_engine("FE")(cfg, "Test")
        res.append(eng.test(batches=3))
    assert torch.equal(res[0]["labels"], res[1]["labels"])
    err = float((res[0]["scores"].double() - res[1]["scores"].double()).abs().max())
    assert within("test() scores, inference_graph on vs off", err, 1e-4)
