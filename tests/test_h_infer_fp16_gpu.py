"""GPU: the fp16 inference runner (InferenceRunner(model, batch, size, "fp16"), UDEB4): the eval forward with the MBConv trunk in
half storage (mbconv.mbconv_eval_half) captured as one hipGraph.

Bars: a reduced-precision mode is held to the float64 oracle by the rule tests/test_e_mixed_precision_gpu.py uses for training —
each output's relative L2 deviation within max(4 x the deviation that ONE fp16 rounding of the parameters and the input causes in
the float64 oracle, 2e-3).  Replays, the follow-the-model property and the engine hook are bitwise.
"""
import copy
import ctypes

import pytest
import torch

from oracle import eb4, param_fill
from tests import oracle_util as ou
from tests.margins import within
from tests.test_c_model_gpu import _model

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _flat(out):
    ld = out["loss_dict"]
    d = {"cls_out": out["cls_out"], "rec": out["rec"]}
    for k in ("factorization", "freq_mask", "spat_mask", "spatial", "freq"):
        d[k] = ld[k]
    for i, t in enumerate(ld["triplet"]):
        d[f"triplet{i}"] = t
    return d


def _clone(out):
    return {k: v.detach().clone() for k, v in _flat(out).items()}


def _replayed(m, x, precision="fp16"):
    from unidefense_amd.infer import InferenceRunner
    r = InferenceRunner(m, x.shape[0], x.shape[-1], precision)
    r(x)
    out = r(x)
    assert r.graph is not None
    return r, out


def _rl2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ---- 1. whole model against the float64 oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,size", [(4, 256), (2, 380)])
def test_fp16_runner_vs_float64_oracle(n, size):
    dev = _dev()
    ou.fit_cpu_threads()
    m = _model(dev, 0.0, 0.3).eval()
    x = param_fill.make_input(n, size, 61)
    _, out = _replayed(m, x.to(dev))
    got = _clone(out)
    for v in got.values():
        assert v.dtype == torch.float32 and torch.isfinite(v).all()
    sd = {k: v.detach().double() for k, v in ou.oracle_state(0.0, 0.3).items()}
    params = {k for k, _ in m.named_parameters()}
    sd16 = {k: (v.half().double() if k in params else v) for k, v in sd.items()}
    with torch.no_grad():
        ref = _flat(eb4.forward_eb4(sd, x.double(), training=False))
        yard = _flat(eb4.forward_eb4(sd16, x.half().double(), training=False))
    ok = []
    for k in ref:
        y = _rl2(yard[k], ref[k])
        e = _rl2(got[k], ref[k])
        bar = max(4.0 * y, 2e-3)
        print(f"  {k}: fp16 runner {e:.2e}  yardstick {y:.2e}  bar {bar:.2e}")
        ok.append(within(f"fp16 runner vs float64 oracle {size}^2: {k} / bar", e / bar, 1.0))
    assert all(ok)


# ---- 2. replays, and a runner that follows the model ------------------------------------------------------------------------
def test_fp16_replay_bitwise_and_follows_optimizer_step():
    dev = _dev()
    from unidefense_amd.infer import InferenceRunner
    m = _model(dev, 0.0, 0.3).eval()
    x = param_fill.make_input(4, 256, 71).to(dev)
    r, out = _replayed(m, x)
    a = _clone(out)
    b = _flat(r(x))
    assert all(torch.equal(a[k], b[k]) for k in a)
    torch.manual_seed(7)
    params = [p for p in m.parameters() if p.requires_grad]
    for p in params:
        p.grad = torch.randn_like(p) * 1e-2
    opt = torch.optim.AdamW(params, lr=1e-3)
    opt.step()
    for blk in (m.backbone._blocks[3], m.backbone._blocks[12]):      # an expanding block and a spectral block
        blk._bn0.running_mean.add_(0.05)
        blk._bn1.running_var.mul_(1.5)
    m.backbone._bn0.running_mean.add_(0.02)                            # the stem's, applied on block 0's load
    after = _clone(r(x))
    fresh = InferenceRunner(m, 4, 256, "fp16")
    fresh(x)
    ref = _flat(fresh(x))
    assert _rl2(after["cls_out"], a["cls_out"]) > 1e-2                 # the step changed the function
    bad = [k for k in ref if not torch.equal(after[k], ref[k])]
    assert not bad, bad


def test_fp16_runner_leaves_gemm_path_and_fp32_runner_unchanged():
    dev = _dev()
    from unidefense_amd import lib
    m = _model(dev, 0.0, 0.3).eval()
    x = param_fill.make_input(2, 256, 81).to(dev)
    path = lib.call("ud_gemm_get_path")
    r32, out32 = _replayed(m, x, "fp32")
    a = _clone(out32)
    _, out16 = _replayed(m, x, "fp16")
    assert lib.call("ud_gemm_get_path") == path
    b = _flat(r32(x))
    assert all(torch.equal(a[k], b[k]) for k in a)
    with torch.no_grad():                                               # the eager eval forward does not take the half path
        e = _flat(m(x))
    assert _rl2(e["cls_out"], a["cls_out"]) < 1e-5
    assert lib.call("ud_gemm_get_path") == path


def test_fp16_runner_samples_permute_bs96():
    dev = _dev()
    m = _model(dev, 0.0, 0.3).eval()
    x = param_fill.make_input(96, 256, 91).to(dev)
    r, out = _replayed(m, x)
    cls, rec = out["cls_out"].clone(), out["rec"].clone()
    perm = torch.randperm(96, generator=torch.Generator().manual_seed(3)).to(dev)
    o = r(x[perm].contiguous())
    wc = float((o["cls_out"] - cls[perm]).abs().max() / cls.abs().max())
    wr = float((o["rec"] - rec[perm]).abs().max() / rec.abs().max())
    print(f"  permuted batch: cls_out {wc:.2e}  rec {wr:.2e}")
    assert within("fp16 bs-96 permuted replay, cls_out", wc, 1e-5)
    assert within("fp16 bs-96 permuted replay, rec", wr, 1e-4)


# ---- 3. interface -----------------------------------------------------------------------------------------------------------
def test_fp16_runner_interface():
    dev = _dev()
    m = _model(dev, 0.0, 0.3).eval()
    r32 = m.inference_runner(2, 256)
    r16 = m.inference_runner(2, 256, "fp16")
    assert r16 is not r32 and r16.precision == "fp16" and r32.precision == "fp32"
    assert m.inference_runner(2, 256, "fp32") is r32 and m.inference_runner(2, 256, precision="fp16") is r16
    assert set(m._ud_runners) == {(2, 256), (2, 256, "fp16")}
    with pytest.raises(ValueError, match="differs"):
        r16(torch.zeros(2, 3, 256, 256, device=dev, dtype=torch.float16))
    with pytest.raises(ValueError, match="precision"):
        m.inference_runner(2, 256, "bf16")
    for i in range(4):                                                  # the eviction rule counts both precisions
        m.inference_runner(1, 64 + 32 * i, "fp16")
    assert len(m._ud_runners) == 4 and (2, 256) not in m._ud_runners and (2, 256, "fp16") not in m._ud_runners
    assert r16.calls == 0


def test_engine_test_with_fp16_inference():
    _dev()
    from tests.test_d_train_engine import CONFIG
    from unidefense_amd.engine import get_engine
    torch.manual_seed(0)
    cfg = copy.deepcopy(CONFIG)
    cfg["config"]["inference_graph"] = True
    cfg["config"]["inference_precision"] = "fp16"
    eng = get_engine("FE")(cfg, "Test")
    res = eng.test(batches=3)
    m = eng.model_without_ddp
    assert any(len(k) == 3 and k[2] == "fp16" for k in m._ud_runners)
    scores = []
    for step in range(1, 4):
        xr, _, xf, _ = eng.test_iterator(step, eng.batch, eng.size, eng.device)
        x = torch.cat([xr, xf], 0).contiguous()
        scores.append(torch.softmax(m.inference_runner(x.shape[0], x.shape[-1], "fp16")(x)["cls_out"], 1)[:, 0])
    assert torch.equal(res["scores"].cpu(), torch.cat(scores).cpu())


# ---- 4. statistics off in eval ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [8, 16, 32, 12, 24])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_irfft2_mix_without_statistics(S, dtype):
    """ud_irfft2_mix / ud_irfft2_two_pass with sum == sumsq == NULL: the same mix and difference, no statistics epilogue"""
    dev = _dev()
    from unidefense_amd import kernels as K
    N, C = 2, 64
    g = torch.Generator().manual_seed(S)
    Y = torch.randn(N, S, S // 2 + 1, 2 * C, generator=g).to(dev, dtype)
    spat = torch.randn(N, S, S, C, generator=g).to(dev, dtype)
    alpha = torch.tensor(0.3, device=dev)
    acc = torch.zeros(2 * C, dtype=torch.float64, device=dev)
    y1, f1 = K.irfft2_mix(Y, 1.0 / S, spat, alpha, acc)
    y0, f0 = K.irfft2_mix(Y, 1.0 / S, spat, alpha, None)
    torch.cuda.synchronize()
    assert torch.equal(y0, y1) and torch.equal(f0, f1)
    assert float((acc[:C] - y1.double().sum((0, 1, 2))).abs().max()) < 1e-6 * float(y1.double().abs().sum())


# ---- 5. the half-storage eval node (ud_mb_eval_dw_h) against float64 --------------------------------------------------------
def _node_shapes():
    import math
    from unidefense_amd import kernels as K
    from unidefense_amd.model.arch import build_arch
    shapes = set()
    for size in (256, 380):
        arch = build_arch("efficientnet-b4", "ortho", size)
        s = math.ceil(size / 2)
        for sp in arch["blocks"]:
            if sp.expand != 1 and sp.sf_norm is None:
                assert K.mb_eval_dw_h_ok(sp.cin, sp.cexp, sp.k, sp.stride), (sp.cin, sp.cexp, sp.stride)
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


def test_node_h_shapes_cover_the_blocks():
    sh = _node_shapes() if torch.cuda.is_available() else []
    if not sh:
        pytest.skip("needs a GPU")
    assert {s[4] for s in sh} == {1, 2} and {s[1] for s in sh} == {24, 32, 272, 448}
    assert {s[0] for s in sh} >= {128, 64, 8, 190, 95, 12}, sh


@pytest.mark.parametrize("shape", _node_shapes() if torch.cuda.is_available() else [], ids=str)
def test_mb_eval_dw_h_vs_float64(shape):
    """d (both out_act forms) within 2e-3 of max |ref| — one fp16 rounding of the output — and the SE pool within 1e-3 relative,
    against conv1x1 -> BN -> swish -> SAME-padded depthwise -> BN -> swish in float64 on fp16-representable inputs and expand
    weights; the running buffers are not written"""
    import torch.nn.functional as F
    dev = _dev()
    from unidefense_amd import kernels as K
    H, Ci, CE, k, s, pad = shape
    N = 3 if H <= 64 else 2
    g = torch.Generator().manual_seed(H * 7 + Ci + s)
    x = torch.randn(N, H, H, Ci, generator=g).half().float()
    we = (torch.randn(CE, Ci, generator=g) / Ci ** 0.5).half().float()
    w = torch.randn(CE, 1, k, k, generator=g) / k
    bn0, bn1 = _bn_mod(CE, dev, 1), _bn_mod(CE, dev, 2)
    keep = [t.clone() for t in (bn0.running_mean, bn0.running_var, bn1.running_mean, bn1.running_var)]
    pl, pr, pt, pb = pad
    Ho, Wo = (H + pt + pb - k) // s + 1, (H + pl + pr - k) // s + 1
    xd, wed, wtd = x.to(dev).half().contiguous(), we.to(dev), w.view(CE, k * k).t().contiguous().to(dev)
    d1, pool1 = K.mb_eval_dw_h(xd, wed, K.EvalBN(bn0, 1), wtd, K.EvalBN(bn1, 1), k, s, pt, pl, Ho, Wo, out_act=True)
    d0, pool0 = K.mb_eval_dw_h(xd, wed, K.EvalBN(bn0, 1), wtd, K.EvalBN(bn1, 1), k, s, pt, pl, Ho, Wo, out_act=False)
    torch.cuda.synchronize()
    assert d1.dtype == torch.float16 and d0.dtype == torch.float16
    for a_, b_ in zip(keep, (bn0.running_mean, bn0.running_var, bn1.running_mean, bn1.running_var)):
        assert torch.equal(a_, b_)

    def bn64(z, bn):
        ga, be = bn.weight.double().cpu(), bn.bias.double().cpu()
        mu, var = bn.running_mean.double().cpu(), bn.running_var.double().cpu()
        return (z - mu.view(1, -1, 1, 1)) / torch.sqrt(var + bn.eps).view(1, -1, 1, 1) * ga.view(1, -1, 1, 1) + be.view(1, -1, 1, 1)
    x64 = x.double().permute(0, 3, 1, 2)
    z0 = bn64(F.conv2d(x64, we.double().view(CE, Ci, 1, 1)), bn0)
    e = z0 * torch.sigmoid(z0)
    dw = F.conv2d(F.pad(e, (pl, pr, pt, pb)), w.double(), stride=s, groups=CE)
    z1 = bn64(dw, bn1)
    d = z1 * torch.sigmoid(z1)
    g0, g1 = d0.double().cpu().permute(0, 3, 1, 2), d1.double().cpu().permute(0, 3, 1, 2)
    r0 = float((g0 - dw).abs().max() / dw.abs().max())
    r1 = float((g1 - d).abs().max() / d.abs().max())
    pref = d.mean((2, 3))
    rp1 = float((pool1.double().cpu() - pref).abs().max() / pref.abs().max())
    rp0 = float((pool0.double().cpu() - pref).abs().max() / pref.abs().max())
    print(f"  {shape} N={N}: raw {r0:.2e}  act {r1:.2e}  pool {rp1:.2e} / {rp0:.2e}")
    assert within(f"ud_mb_eval_dw_h raw {shape}", r0, 2e-3)
    assert within(f"ud_mb_eval_dw_h act {shape}", r1, 2e-3)
    assert within(f"ud_mb_eval_dw_h pool (out_act 1) {shape}", rp1, 1e-3)
    assert within(f"ud_mb_eval_dw_h pool (out_act 0) {shape}", rp0, 1e-3)


def test_mb_eval_dw_h_refuses_training_form_bn():
    dev = _dev()
    from unidefense_amd import kernels as K, lib
    N, H, Ci, CE = 2, 8, 32, 192
    bn = _bn_mod(CE, dev, 4)
    x = torch.zeros(N, H, H, Ci, device=dev, dtype=torch.float16)
    we = torch.zeros(CE, Ci, device=dev)
    wt = torch.zeros(9, CE, device=dev)
    d = torch.empty(N, H, H, CE, device=dev, dtype=torch.float16)
    part = torch.empty(N, 1, CE, device=dev)
    acc = torch.zeros(2 * CE, dtype=torch.float64, device=dev)
    train = K.DeferredBN(acc, CE, N * H * H, bn.weight, bn.bias, bn.eps, 1)
    ev = K.EvalBN(bn, 1)
    h = lib.load()
    for b0, b1 in ((train, ev), (ev, train)):
        st = h.ud_mb_eval_dw_h(K._p(x), K._p(we), ctypes.byref(b0.ref()), K._p(wt), ctypes.byref(b1.ref()), K._p(d), K._p(part),
                               N, H, H, Ci, CE, H, H, 3, 1, 1, 1, 0, K._stream())
        assert st == -1000
    assert h.ud_mb_eval_dw_h(K._p(x), K._p(we), ctypes.byref(ev.ref()), K._p(wt), ctypes.byref(ev.ref()), K._p(d), K._p(part),
                             N, H, H, Ci, CE, H, H, 3, 1, 1, 1, 0, K._stream()) == 0
    torch.cuda.synchronize()


# ---- 6. stage-local against the float64 oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("node", [False, True], ids=["composed", "node"])
@pytest.mark.parametrize("stage", [1, 2, 3, 4, 5, 6])
def test_fp16_eval_stage_local_vs_float64_oracle(stage, node):
    """every backbone stage's blocks on the fp16 eval path (mbconv.mbconv_eval_half, with the model's node threshold) fed the float64
    oracle's own eval-mode input of that stage rounded once to fp16, against oracle/eb4.py:mbconv(training=False) in float64 on the
    same rounded input: relative L2 of the output <= 3e-3.  node: the expanding non-SF blocks on ud_mb_eval_dw_h (the model's
    threshold keeps them on the composed half kernels, which measured faster)"""
    dev = _dev()
    from unidefense_amd import kernels as K
    from unidefense_amd import mbconv as MB
    from unidefense_amd import tape as T
    ou.fit_cpu_threads()
    x = param_fill.make_input(4, 256, 38)
    sd = ou.oracle_state(0.0, 0.3, dtype=torch.float64)
    arch = eb4.eb4_arch(freq_norm="ortho")
    delim = arch["delimiter"]
    with torch.no_grad():
        feats = eb4.forward_eb4(sd, x.double(), training=False)["_feats"]
        src = {1: "x_b0", 2: "x_b1", 3: "x_b2", 4: "x_b3", 5: "x_b4", 6: "att_out"}[stage]
        h64 = feats[src].half().double()
        h = h64
        for idx in range(delim[stage - 1], delim[stage]):
            h = eb4.mbconv(h, sd, f"backbone._blocks.{idx}", arch["blocks"][idx], False, arch["bn_eps"])
        m = _model(dev, 0.0, 0.3).eval()
        m.EVAL_NODE_H_MAX_CIN = 448 if node else 0
        pix = lambda t: t.permute(0, 2, 3, 1).contiguous()
        K.begin_forward(m)
        try:
            ws = [blk._depthwise_conv.weight for blk in m.backbone._blocks]
            wts = K.dw_weights_tapmajor(ws)
            T.DW_WT = {id(w): (w, w._version, wts[id(w)]) for w in ws}
            out = m._blocks(None, pix(h64).to(dev).half(), stage, {"drop_connect": {}}, MB.TrunkMode(MB.HALF, wts))
        finally:
            K.end_forward()
        torch.cuda.synchronize()
    assert out.dtype == torch.float16
    e = _rl2(out, pix(h))
    print(f"  stage {stage} (blocks {delim[stage - 1]}..{delim[stage] - 1}): output relative L2 {e:.2e}")
    assert within(f"fp16 eval stage {stage}: output relative L2", e, 3e-3)
