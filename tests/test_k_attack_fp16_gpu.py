"""GPU: the fp16 input-gradient / attack runners (InputGradRunner / AttackRunner with precision="fp16", UDEB4) and the frozen half
backward under them: the entry points that REQUIRE the eval form of ud_bn_ref (ud_coldot_bn_eval, ud_se_scale_bwd_bn_eval,
ud_bn_eval_bwd, ud_dwtile_dgrad_eval, ud_sfmix_pool_bwd) and the tape node mbconv.mbconv_frozen_half.

Bars.  Kernels: the project's own for these kernel families (tests/test_b_fused_kernels_gpu.py) — relative L2 2e-5 in fp32 storage,
1e-3 in half storage (one fp16 rounding of the result) — against float64 restatements written here with torch autograd on
fp16-representable inputs.  Stage-local: 3e-3 (output) / 5e-3 (input gradient), the bars of the stage-local half-storage training
test.  Whole model: max(4 x yardstick, 5e-3) on relative L2 and on max|d| / max|ref|, the yardstick being what ONE fp16 rounding of
the parameters and the input does to the float64 oracle's own gradient (the rule of test_fp16_runner_vs_float64_oracle).  Attack:
the three checks of tests/test_j_attack_gpu.py at precision="fp16" (formula bitwise, budgets exact, gain >= 0.9 of the oracle's).

Observed on an MI355X (this file's own prints): see DESIGN 3l."""
import copy
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import eb4, losses as OL, param_fill
from tests import oracle_util as ou
from tests.margins import within
from tests.test_attack_cpu import ref_sample_sumsq, ref_step_linf

pytestmark = pytest.mark.gpu

LO, HI = -1.0, 1.0
EPS2 = 2.0 / 255.0
BAR32, BAR16 = 2e-5, 1e-3


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    ou.fit_cpu_threads()
    return torch.device("cuda:0")


def _build(dev):
    from unidefense_amd.model import load_model
    m = load_model("UDEB4")(num_classes=2, drop_rate=0.5, extractor="efficientnet-b4")
    param_fill.fill_module_(m, sf_coef=0.0, fuse_coef=0.3)
    return m.to(dev)


_MODEL = []


def _shared(dev):
    if not _MODEL:
        _MODEL.append(_build(dev).eval())
    return _MODEL[0]


def _rl2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _errs(g, ref):
    g, ref = g.detach().double().cpu(), ref.detach().double().cpu()
    d = g - ref
    return float(d.abs().max() / ref.abs().max()), float(d.norm() / ref.norm())


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
    """the eval BatchNorm of a pixel-major float64 tensor [..., C]"""
    ga, be = bn.weight.detach().double().cpu(), bn.bias.detach().double().cpu()
    mu, var = bn.running_mean.double().cpu(), bn.running_var.double().cpu()
    return (z - mu) / torch.sqrt(var + bn.eps) * ga + be


def _swish(z):
    return z * torch.sigmoid(z)


def _h(t):
    """fp16-representable fp32 values"""
    return t.half().float()


def _store(t, dev, dtype):
    return t.to(dev).to(dtype).contiguous()


# ---- 1. kernels against float64 ---------------------------------------------------------------------------------------------
# (N, map side, expanded channels): Ce 144 / 192 / 1632 on the 64 x 64 and 8 x 8 maps of the 256 x 256 trunk, 95 x 95 of the 380 x 380 one
EW_SHAPES = [(2, 64, 144), (2, 64, 192), (3, 8, 1632), (1, 95, 192), (32, 8, 1632)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("N,S,C", EW_SHAPES)
def test_coldot_bn_eval_vs_float64(N, S, C, dtype):
    from unidefense_amd import kernels as K
    dev = _dev()
    g = torch.Generator().manual_seed(N + S + C)
    HW = S * S
    d, dc = _h(torch.randn(N, S, S, C, generator=g)), _h(torch.randn(N, S, S, C, generator=g))
    bn = _bn_mod(C, dev, 3)
    keep = [bn.running_mean.clone(), bn.running_var.clone()]
    ref = (dc.double() * _swish(_bn64(d.double(), bn))).sum((1, 2))
    dd, dcd = _store(d, dev, dtype), _store(dc, dev, dtype)
    outs = []
    for _ in range(2):
        out = torch.zeros(N * C, dtype=torch.float64, device=dev)
        K.coldot_bn_eval(dcd, dd, K.EvalBN(bn, 1), N, HW, out)
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])                                # no atomics shared by workgroups: run to run bitwise
    assert torch.equal(keep[0], bn.running_mean) and torch.equal(keep[1], bn.running_var)
    e = _rl2(outs[0].view(N, C), ref)
    print(f"  ud_coldot_bn_eval {N}x{S}x{S}x{C} {dtype}: relative L2 {e:.2e}")
    # fp64 sums of fp32 products of the stored operands, in either storage: the fp32 bar
    assert within(f"ud_coldot_bn_eval {(N, S, C)} {dtype}: relative L2", e, BAR32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("N,S,C", EW_SHAPES)
def test_se_scale_bwd_bn_eval_vs_float64(N, S, C, dtype):
    from unidefense_amd import kernels as K
    dev = _dev()
    g = torch.Generator().manual_seed(2 * N + S + C)
    HW = S * S
    d, dc = _h(torch.randn(N, S, S, C, generator=g)), _h(torch.randn(N, S, S, C, generator=g))
    s2, dpool = torch.randn(N, C, generator=g), torch.randn(N, C, generator=g) * HW ** 0.5
    bn = _bn_mod(C, dev, 4)
    d64 = d.double().requires_grad_()
    a = _swish(_bn64(d64, bn))
    gate = torch.sigmoid(s2.double()).view(N, 1, 1, C)
    (a * gate * dc.double()).sum().add((a * (dpool.double() / HW).view(N, 1, 1, C)).sum()).backward()
    got = K.se_scale_bwd_bn_eval(_store(dc, dev, dtype), _store(d, dev, dtype), K.EvalBN(bn, 1), s2.to(dev), dpool.to(dev), 1.0 / HW,
                                 N, HW)
    torch.cuda.synchronize()
    assert got.dtype == dtype
    e = _rl2(got, d64.grad)
    print(f"  ud_se_scale_bwd_bn_eval {N}x{S}x{S}x{C} {dtype}: relative L2 {e:.2e}")
    assert within(f"ud_se_scale_bwd_bn_eval {(N, S, C)} {dtype}: relative L2", e, BAR32 if dtype == torch.float32 else BAR16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("N,S,C", [(2, 64, 24), (3, 8, 272), (1, 95, 56), (2, 64, 144)])
def test_bn_eval_bwd_vs_float64(N, S, C, act, dtype):
    from unidefense_amd import kernels as K
    dev = _dev()
    g = torch.Generator().manual_seed(N + 3 * S + C + act)
    x, dy = _h(torch.randn(N, S, S, C, generator=g)), _h(torch.randn(N, S, S, C, generator=g))
    bn = _bn_mod(C, dev, 5)
    x64 = x.double().requires_grad_()
    z = _bn64(x64, bn)
    ((_swish(z) if act else z) * dy.double()).sum().backward()
    got = K.bn_eval_bwd(_store(dy, dev, dtype), _store(x, dev, dtype) if act else None, K.EvalBN(bn, act), 1, N * S * S)
    torch.cuda.synchronize()
    e = _rl2(got, x64.grad)
    print(f"  ud_bn_eval_bwd {N}x{S}x{S}x{C} act {act} {dtype}: relative L2 {e:.2e}")
    assert within(f"ud_bn_eval_bwd {(N, S, C)} act {act} {dtype}: relative L2", e, BAR32 if dtype == torch.float32 else BAR16)


def _dw_cases():
    from unidefense_amd.model.arch import same_pad
    cases = []
    for (N, S, C) in [(2, 64, 144), (2, 64, 192), (3, 8, 1632), (1, 95, 192)]:
        for k in (3, 5):
            for stride in (1, 2):
                lo, hi = same_pad(S, k, stride)
                # every gate mode and both `add` forms appear for each geometry family; the full cross product on the 8 x 8 map
                combos = [(gm, add) for gm in (0, 1, 2) for add in (False, True)] if S == 8 else \
                    [((k + stride + C) % 3, True), ((k + stride + C + 1) % 3, False)]
                for gm, add in combos:
                    cases.append((N, S, C, k, stride, (lo, hi), gm, add))
    return cases


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("case", _dw_cases(), ids=str)
def test_dwtile_dgrad_eval_vs_float64(case, dtype):
    """dx = (gate dwconv^T(dy) + add) act'(bn(x)) gamma invstd against autograd of gate <conv(swish(bn(x))), dy> + <swish(bn(x)), add>
    in float64 (TF-SAME pads of the real blocks; stride 2 reads dy through the zero-stuffed grid)"""
    from unidefense_amd import kernels as K
    dev = _dev()
    N, S, C, k, stride, (lo, hi), gm, with_add = case
    g = torch.Generator().manual_seed(S * 11 + C + k + stride + gm)
    So = (S + lo + hi - k) // stride + 1
    x = _h(torch.randn(N, S, S, C, generator=g))
    dy = _h(torch.randn(N, So, So, C, generator=g))
    add = _h(torch.randn(N, S, S, C, generator=g)) if with_add else None
    w = torch.randn(C, 1, k, k, generator=g) / k
    alpha = torch.tensor(0.4)
    bn = _bn_mod(C, dev, 6)
    x64 = x.double().requires_grad_()
    a = _swish(_bn64(x64, bn))
    y = F.conv2d(F.pad(a.permute(0, 3, 1, 2), (lo, hi, lo, hi)), w.double(), stride=stride, groups=C)
    sg = float(torch.sigmoid(alpha.double()))
    gate = (1.0, sg, 1.0 - sg)[gm]
    L = gate * (y * dy.double().permute(0, 3, 1, 2)).sum()
    if with_add:
        L = L + (a * add.double()).sum()
    L.backward()
    wt = w.view(C, k * k).t().contiguous().to(dev)
    got = K.dwtile_dgrad_eval(_store(dy, dev, dtype), wt, k, lo, lo, _store(x, dev, dtype), K.EvalBN(bn, 1),
                              alpha.to(dev) if gm else None, gm, _store(add, dev, dtype) if with_add else None, stride)
    torch.cuda.synchronize()
    assert got.dtype == dtype and got.shape == x.shape
    e = _rl2(got, x64.grad)
    print(f"  ud_dwtile_dgrad_eval {case} {dtype}: relative L2 {e:.2e}")
    assert within(f"ud_dwtile_dgrad_eval {case} {dtype}: relative L2", e, BAR32 if dtype == torch.float32 else BAR16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_sfmix_pool_bwd_exact(dtype):
    from unidefense_amd import kernels as K
    dev = _dev()
    dy = _h(torch.randn(3, 12, 12, 56, generator=torch.Generator().manual_seed(2)))
    got = K.sfmix_pool_bwd(_store(dy, dev, dtype))
    want = (dy * 0.25).repeat_interleave(2, 1).repeat_interleave(2, 2).to(dtype)          # a power-of-two factor: exact
    assert torch.equal(got.cpu(), want)


def test_se_bwd_without_weight_gradients_is_the_same_dpool():
    from unidefense_amd import kernels as K
    dev = _dev()
    g = torch.Generator().manual_seed(8)
    N, C, Cs = 4, 1632, 68
    dgate = torch.randn(N, C, generator=g).double().to(dev)
    s2, s1 = torch.randn(N, C, generator=g).to(dev), torch.randn(N, Cs, generator=g).to(dev)
    We, Wr = (torch.randn(C, Cs, generator=g) / 8).to(dev), (torch.randn(Cs, C, generator=g) / 40).to(dev)
    pool = torch.randn(N, C, generator=g).double().to(dev)
    full = K.se_bwd(dgate.view(-1), s2, s1, We, Wr, pool.view(-1), 1.0 / 64)
    lean = K.se_bwd(dgate.view(-1), s2, s1, We, Wr, None, 1.0 / 64, need_w=False)
    torch.cuda.synchronize()
    assert lean[1:] == (None, None, None, None)
    assert within("ud_se_bwd_a / _b without weight gradients: dpool vs the full form, relative L2", _rl2(lean[0], full[0]), 1e-6)


def test_frozen_entry_points_refuse_a_training_form_bn_on_the_device():
    dev = _dev()
    from unidefense_amd import kernels as K, lib
    C, S = 64, 8
    bn = _bn_mod(C, dev, 5)
    x = torch.randn(1, S, S, C, device=dev)
    out = torch.zeros(C, dtype=torch.float64, device=dev)
    acc = torch.zeros(2 * C, dtype=torch.float64, device=dev)
    s = torch.zeros(1, C, device=dev)
    wt = torch.zeros(9, C, device=dev)
    tr = ctypes.byref(K.DeferredBN(acc, C, S * S, bn.weight, bn.bias, bn.eps, 1).ref())
    ev = ctypes.byref(K.EvalBN(bn, 1).ref())
    h, p, st = lib.load(), K._p, K._stream()
    dx = torch.empty_like(x)
    for ref, want in ((tr, -1000), (ev, 0)):
        assert h.ud_coldot_bn_eval(p(x), p(x), ref, 1, S * S, C, K._pd(out), None, 0, st) == want
        assert h.ud_se_scale_bwd_bn_eval(p(x), p(x), ref, p(s), p(s), 1.0, p(dx), 1, S * S, C, 0, st) == want
        assert h.ud_bn_eval_bwd(p(x), p(x), ref, p(dx), 1, S * S, C, 0, st) == want
        assert h.ud_dwtile_dgrad_eval(p(x), p(wt), None, 0, None, p(x), ref, p(dx), 1, S, S, C, S, S, 3, 1, 1, 1, 0, st) == want
    torch.cuda.synchronize()


# ---- 2. stage-local: mbconv.mbconv_frozen_half against the float64 oracle -------------------------------------------------------
@pytest.mark.parametrize("stage", [0, 1, 2, 3, 4, 5, 6])
def test_frozen_half_stage_local_vs_float64_oracle(stage):
    """every backbone stage's blocks on mbconv.mbconv_frozen_half alone, forward and backward, fed the float64 oracle's own eval-mode
    input of that stage rounded once to fp16 (stage 0: the raw stem output, its BatchNorm + swish applied on load) and a seeded
    output gradient, against oracle/eb4.py:mbconv(training=False) autograd in float64 on the same tensors.
    Observed (MI355X): see DESIGN 3l."""
    dev = _dev()
    from unidefense_amd import kernels as K
    from unidefense_amd import mbconv as MB
    from unidefense_amd import tape as T
    x = param_fill.make_input(4, 256, 38)
    sd = ou.oracle_state(0.0, 0.3, dtype=torch.float64)
    arch = eb4.eb4_arch(freq_norm="ortho")
    delim = arch["delimiter"]
    lo, hi = (delim[stage - 1] if stage else 0), delim[stage]
    with torch.no_grad():
        if stage == 0:
            st = arch["stem"]
            src64 = eb4.conv_static_same(x.double(), sd["backbone._conv_stem.weight"], st["s"], st["pad"])
        else:
            feats = eb4.forward_eb4(sd, x.double(), training=False)["_feats"]
            src64 = feats[{1: "x_b0", 2: "x_b1", 3: "x_b2", 4: "x_b3", 5: "x_b4", 6: "att_out"}[stage]]
    h64 = src64.half().double().requires_grad_()
    h = eb4.swish(eb4.batch_norm(h64, sd, "backbone._bn0", False, arch["bn_eps"])) if stage == 0 else h64
    for idx in range(lo, hi):
        h = eb4.mbconv(h, sd, f"backbone._blocks.{idx}", arch["blocks"][idx], False, arch["bn_eps"])
    dout = torch.randn(h.shape, generator=torch.Generator().manual_seed(2000 + stage)).half().double()
    h.backward(dout)

    m = _build(dev).eval()
    pix = lambda t: t.permute(0, 2, 3, 1).contiguous()
    h_pix = pix(h64.detach()).to(dev).half()
    got = {}
    with torch.no_grad():
        K.begin_forward(m)
        try:
            tape = T.Tape()
            tape.wgrad_on = False
            ws = [blk._depthwise_conv.weight for blk in m.backbone._blocks]
            wts = K.dw_weights_tapmajor(ws)
            T.DW_WT = {id(w): (w, w._version, wts[id(w)]) for w in ws}
            lazy = MB.LazyInput(K.EvalBN(m.backbone._bn0, 1), lambda dh: got.update(dx=dh)) if stage == 0 else None
            out = m._blocks(tape, h_pix, stage, {"drop_connect": {}}, MB.TrunkMode(MB.HALF, wts), lazy)
        finally:
            K.end_forward()
        assert len(tape.nodes) == hi - lo                                   # one node per block: no block left the frozen half path
        if stage:
            tape.nodes.insert(0, lambda: got.update(dx=tape.grads.get(id(h_pix))))      # runs last in the reversed replay
        tape.add_grad(out, pix(dout).to(dev).half())
        K.reset_zero_pool()
        tape.backward()
        torch.cuda.synchronize()
    assert out.dtype == torch.float16 and got["dx"].dtype == torch.float16
    assert not tape.param_grads and all(p.grad is None for p in m.parameters())
    e_out, e_dx = _rl2(out, pix(h)), _rl2(got["dx"], pix(h64.grad))
    print(f"  frozen half stage {stage} (blocks {lo}..{hi - 1}): output {e_out:.2e}  input gradient {e_dx:.2e}")
    ok = [within(f"frozen half stage {stage}: output relative L2", e_out, 3e-3),
          within(f"frozen half stage {stage}: input-gradient relative L2", e_dx, 5e-3)]
    assert all(ok)


def test_frozen_half_node_refuses_a_tape_with_weight_gradients():
    dev = _dev()
    from unidefense_amd import mbconv as MB, tape as T
    m = _shared(dev)
    tape = T.Tape()                                                           # wgrad_on True: a training tape
    x = torch.zeros(1, 8, 8, m.backbone._blocks[30].spec.cin, device=dev, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="FROZEN"):
        MB.mbconv_frozen_half(tape, x, m.backbone._blocks[30], None)


# ---- 3. whole model against the float64 oracle --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _states():
    sd = {k: v.detach().double() for k, v in ou.oracle_state(0.0, 0.3).items()}
    shapes = eb4.eb4_state_shapes(2)
    params = {k for k in shapes if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    sd16 = {k: (v.half().double() if k in params and v.dtype.is_floating_point else v) for k, v in sd.items()}
    return sd, sd16


def _loss64(sd, x64, y):
    return F.cross_entropy(eb4.forward_eb4(sd, x64, training=False)["cls_out"], y, reduction="sum")


def _grad64(sd, x64, y):
    xg = x64.detach().clone().requires_grad_()
    g, = torch.autograd.grad(_loss64(sd, xg, y), xg)
    return g


def _flat(out):
    ld = out["loss_dict"]
    d = {"cls_out": out["cls_out"], "rec": out["rec"]}
    for k in ("factorization", "freq_mask", "spat_mask", "spatial", "freq"):
        d[k] = ld[k]
    for i, t in enumerate(ld["triplet"]):
        d[f"triplet{i}"] = t
    return d


@pytest.mark.parametrize("size,n,seed", [(256, 1, 7), (256, 2, 7), (380, 1, 7)])
def test_fp16_input_grad_runner_vs_float64_oracle(size, n, seed):
    """Observed (MI355X): see DESIGN 3l."""
    from unidefense_amd import lib, mbconv as MB
    from unidefense_amd.attack import InputGradRunner
    from unidefense_amd.infer import InferenceRunner
    dev = _dev()
    m = _shared(dev)
    x = param_fill.make_input(n, size, seed)
    y = param_fill.make_labels(n)
    xd, yd = x.to(dev), y.to(dev)
    sd, sd16 = _states()
    ref = _grad64(sd, x.double(), y)
    yard = _grad64(sd16, x.half().double(), y)
    ymx, yl2 = _errs(yard, ref)
    bar_mx, bar_l2 = max(4.0 * ymx, 5e-3), max(4.0 * yl2, 5e-3)
    path = lib.call("ud_gemm_get_path")
    r = InputGradRunner(m, n, size, precision="fp16")
    assert r.grad_scale == 1024.0
    peak = {}

    def probe(blk, name, t):
        v = float(t.float().abs().max())
        if not v <= peak.get("v", -1.0):
            peak.update(v=v, where=name)
    MB.HALF_GRAD_PROBE = probe
    try:
        eager = r(xd, yd).clone()                                            # the eager warm-up: the probe may synchronise
    finally:
        MB.HALF_GRAD_PROBE = None
    reps = [r(xd, yd).clone() for _ in range(3)]
    out16 = {k: v.clone() for k, v in _flat(r.out).items()}
    torch.cuda.synchronize()
    assert r.graph is not None and r.calls == 4
    assert lib.call("ud_gemm_get_path") == path
    assert torch.isfinite(reps[0]).all() and reps[0].dtype == torch.float32
    assert all(torch.equal(a, reps[0]) for a in reps[1:])
    assert math.isfinite(peak["v"]) and peak["v"] < 65504.0
    print(f"  UDEB4 {size} n={n}: largest scaled (x1024) half gradient of the trunk {peak['v']:.4g} ({peak['where']}), "
          f"headroom to 65504: x{65504.0 / peak['v']:.3g}")
    mx, l2 = _errs(reps[0], ref)
    print(f"  UDEB4 {size} n={n} fp16: max|d|/max|ref| {mx:.2e} (yardstick {ymx:.2e}, bar {bar_mx:.2e})  "
          f"rel L2 {l2:.2e} (yardstick {yl2:.2e}, bar {bar_l2:.2e})")
    # the forward is the fp16 InferenceRunner's, bit for bit
    inf = InferenceRunner(m, n, size, "fp16")
    inf(xd)
    want = _flat(inf(xd))
    bad = [k for k in want if not torch.equal(want[k], out16[k])]
    assert not bad, bad
    # another loss scale: the same gradient within the bar (a missing unscale would be off by a factor 4)
    r12 = InputGradRunner(m, n, size, precision="fp16", grad_scale=2 ** 12)
    r12(xd, yd)
    g12 = r12(xd, yd).clone()
    smx, sl2 = _errs(g12, reps[0])
    print(f"    grad_scale 4096 vs 1024: max|d|/max {smx:.2e}  rel L2 {sl2:.2e}")
    ok = [within(f"fp16 InputGradRunner {size} n={n} vs oracle, max|d| / max|ref| / bar", mx / bar_mx, 1.0),
          within(f"fp16 InputGradRunner {size} n={n} vs oracle, rel L2 / bar", l2 / bar_l2, 1.0),
          within(f"fp16 InputGradRunner {size} n={n} replay vs eager warm-up, rel L2", _rl2(reps[0], eager), 1e-5),
          within(f"fp16 InputGradRunner {size} n={n} grad_scale 4096 vs 1024, max|d| / max / bar", smx / bar_mx, 1.0),
          within(f"fp16 InputGradRunner {size} n={n} grad_scale 4096 vs 1024, rel L2 / bar", sl2 / bar_l2, 1.0)]
    assert all(ok)
    assert all(p.grad is None for p in m.parameters())


def test_fp16_input_grad_runner_permuted_batch():
    from unidefense_amd.attack import InputGradRunner
    dev = _dev()
    m = _shared(dev)
    x = param_fill.make_input(8, 256, 13).to(dev)
    y = param_fill.make_labels(8).to(dev)
    perm = torch.tensor([5, 2, 7, 0, 3, 6, 1, 4], device=dev)
    r = InputGradRunner(m, 8, 256, precision="fp16")
    r(x, y)
    g = r(x, y).clone()
    gp = r(x[perm].contiguous(), y[perm].contiguous()).clone()
    # no step of the frozen pass mixes samples (eval BatchNorms, per-sample SE sums): the bar of the fp32 runner's test
    assert within("fp16 InputGradRunner bs-8 permuted batch vs permuted gradient, rel L2", _rl2(gp, g[perm]), 1e-5)


def test_fp16_runner_keeps_a_nonfinite_gradient_visible():
    from unidefense_amd.attack import AttackRunner
    dev = _dev()
    m = _shared(dev)
    x = param_fill.make_input(1, 256, 7).to(dev)
    y = param_fill.make_labels(1).to(dev)

    def nan_objective(out, yy):
        return F.cross_entropy(out["cls_out"], yy, reduction="sum") * float("nan")
    r = AttackRunner(m, 1, 256, norm="linf", eps=EPS2, steps=1, objective=nan_objective, precision="fp16")
    r(x, y)
    xa = r(x, y)
    bad = torch.isnan(r.g)
    assert bool(bad.any()) and bool(torch.isnan(xa[bad]).all())               # ud_attack_step_linf passes a NaN through


# ---- 4. the attack -----------------------------------------------------------------------------------------------------------
def test_fp16_fgsm_is_the_formula_on_the_runners_own_gradient():
    from unidefense_amd.attack import AttackRunner, InputGradRunner
    dev = _dev()
    m = _shared(dev)
    n, size = 2, 256
    x = param_fill.make_input(n, size, 7).to(dev)
    y = param_fill.make_labels(n).to(dev)
    r = AttackRunner(m, n, size, norm="linf", eps=EPS2, steps=1, precision="fp16")
    assert r.step == EPS2 and r.args["precision"] == "fp16" and r.args["grad_scale"] == 1024.0
    r(x, y)
    xa = r(x, y).clone()
    assert r.graph is not None
    assert torch.equal(xa, ref_step_linf(x, x, r.g, EPS2, EPS2, LO, HI))
    assert float((xa - x).abs().max()) > 0.5 * EPS2
    ig = InputGradRunner(m, n, size, precision="fp16")
    ig(x, y)
    assert within("fp16 AttackRunner.g vs fp16 InputGradRunner, rel L2", _rl2(r.g, ig(x, y)), 1e-5)


@pytest.mark.parametrize("norm", ["linf", "l2"])
def test_fp16_attack_stays_inside_its_budget(norm):
    from unidefense_amd.attack import AttackRunner
    dev = _dev()
    m = _shared(dev)
    n, size, steps = 2, 256, 3
    x = param_fill.make_input(n, size, 7).to(dev)
    y = param_fill.make_labels(n).to(dev)
    assert float(x.min()) >= LO and float(x.max()) <= HI
    eps = EPS2 if norm == "linf" else 0.5
    r = AttackRunner(m, n, size, norm=norm, eps=eps, steps=steps, precision="fp16")
    warm = r(x, y).clone()
    runs = [r(x, y).clone() for _ in range(2)]
    torch.cuda.synchronize()
    assert r.graph is not None and torch.equal(runs[0], runs[1])
    per = 3 * size * size
    for xa in (warm, runs[0]):
        assert torch.isfinite(xa).all()
        assert float(xa.min()) >= LO and float(xa.max()) <= HI
        if norm == "linf":
            assert bool((xa >= x - eps).all()) and bool((xa <= x + eps).all())
            assert float((xa - x).abs().max()) > 0.5 * eps
        else:
            nrm = torch.sqrt(ref_sample_sumsq(xa.cpu(), x.cpu()))
            slack = 2.0 ** -23 * per ** 0.5
            assert bool((nrm <= eps + slack).all()), (nrm, eps)
            assert bool((nrm > 0.1 * eps).all()), nrm


# the UDEB4 rows of tests/test_j_attack_gpu.py's EFFECT.  The bar 0.9 on gain_gpu / gain_ref is consistent with the gradient bar: in
# the oracle's FGSM on make_input(1, 256, 7) at 2/255, Gaussian gradient noise of 4 x the yardstick's norm keeps 0.988 of the gain,
# 16 x keeps 0.878, a one-rounding gradient 1.00001
EFFECT = [(256, 1, 7, "linf", EPS2, 1, EPS2), (256, 1, 7, "linf", EPS2, 3, 1.0 / 255.0), (256, 1, 7, "l2", 1.0, 3, 0.5)]


def _oracle_attack(sd, x, y, norm, eps, steps, step):
    from tests.test_attack_cpu import ref_project_l2, ref_step_l2
    x0 = x.double()
    xa = x0.clone()
    for _ in range(steps):
        g = _grad64(sd, xa, y)
        if norm == "linf":
            xa = ref_step_linf(xa, x0, g, step, eps, LO, HI)
        else:
            xa, _ = ref_step_l2(xa, g, step)
            xa, _ = ref_project_l2(xa, x0, eps, LO, HI)
    return xa


@pytest.mark.parametrize("size,n,seed,norm,eps,steps,step", EFFECT)
def test_fp16_attack_effect_judged_by_the_oracle(size, n, seed, norm, eps, steps, step):
    """Observed (MI355X): see DESIGN 3l."""
    from unidefense_amd.attack import AttackRunner
    dev = _dev()
    m = _shared(dev)
    sd, _ = _states()
    x = param_fill.make_input(n, size, seed)
    y = param_fill.make_labels(n)
    r = AttackRunner(m, n, size, norm=norm, eps=eps, steps=steps, step=step, precision="fp16")
    r(x.to(dev), y.to(dev))
    xa = r(x.to(dev), y.to(dev)).cpu()
    with torch.no_grad():
        base = float(_loss64(sd, x.double(), y))
        gain_gpu = float(_loss64(sd, xa.double(), y)) - base
    xr = _oracle_attack(sd, x, y, norm, eps, steps, step)
    with torch.no_grad():
        gain_ref = float(_loss64(sd, xr, y)) - base
    ratio = gain_gpu / gain_ref
    print(f"  fp16 UDEB4 {norm} eps {eps:.4g} steps {steps}: L64(x) {base:.6g}  gain_ref {gain_ref:.4g}  gain_gpu {gain_gpu:.4g}  "
          f"ratio {ratio:.5f}")
    if steps == 1:
        g64 = _grad64(sd, x.double(), y)
        flips = float((torch.sign(r.g.cpu().double()) != torch.sign(g64)).double().mean())
        print(f"    share of elements whose sign differs from the oracle's: {flips:.4f}")
    assert gain_ref > 0
    assert within(f"fp16 attack effect UDEB4 {norm} steps {steps}: 1 - gain_gpu / gain_ref", 1.0 - ratio, 0.1)


# ---- 5. what the fp16 runners leave alone -------------------------------------------------------------------------------------
def _mixed_flags(m):
    for i, p in enumerate(m.parameters()):
        p.requires_grad_(i % 5 != 0 and p is not getattr(m.bottleneck, "bias", None))
    return [p.requires_grad for p in m.parameters()]


def _train_grads(m, x, tgt):
    n = len(tgt)
    m.train()
    m.zero_grad(set_to_none=True)
    out = m(x, rng=ou.make_rng(n, 32, 0.5))
    OL.pass1_loss(out, tgt, n // 2, n - n // 2, ou.LAMBDAS)["total_loss"].backward()
    torch.cuda.synchronize()
    return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def test_fp16_runners_leave_the_model_and_the_fp32_runners_as_they_were():
    from unidefense_amd import lib
    from unidefense_amd.attack import AttackRunner, InputGradRunner
    dev = _dev()
    n = 2
    x = param_fill.make_input(n, 256, 31).to(dev)
    y = param_fill.make_labels(n).to(dev)
    fresh = _build(dev)
    flags = _mixed_flags(fresh)
    _train_grads(fresh, x, y)                        # the first step of a shape measures GEMM plans; the second runs on them
    want = _train_grads(fresh, x, y)
    del fresh
    m = _build(dev).eval()
    assert _mixed_flags(m) == flags and not all(flags) and any(flags)
    bufs = {k: v.clone() for k, v in m.named_buffers()}
    path = lib.call("ud_gemm_get_path")
    a32 = AttackRunner(m, n, 256, norm="linf", eps=EPS2, steps=2)
    a32(x, y)
    before = a32(x, y).clone()
    for r in (AttackRunner(m, n, 256, norm="linf", eps=EPS2, steps=2, precision="fp16"),
              AttackRunner(m, n, 256, norm="l2", eps=0.5, steps=2, precision="fp16"),
              InputGradRunner(m, n, 256, precision="fp16")):
        for _ in range(3):
            r(x, y)
    torch.cuda.synchronize()
    assert lib.call("ud_gemm_get_path") == path
    assert not m.__dict__.get("_eval_half", False)
    assert [p.requires_grad for p in m.parameters()] == flags
    assert all(p.grad is None for p in m.parameters())
    assert not m.training
    now = dict(m.named_buffers())
    assert all(torch.equal(v, now[k]) for k, v in bufs.items())
    # the fp32 runner captured before: the same x_adv bit for bit, and a fresh fp32 runner agrees with it
    assert torch.equal(a32(x, y), before)
    b32 = AttackRunner(m, n, 256, norm="linf", eps=EPS2, steps=2)
    b32(x, y)
    assert torch.equal(b32(x, y), before)
    got = _train_grads(m, x, y)
    assert got.keys() == want.keys() and len(got) > 300
    diff = [k for k in got if not torch.equal(got[k], want[k])]
    assert not diff, diff[:10]


def test_fp16_captured_runners_follow_an_optimizer_step():
    from unidefense_amd.attack import AttackRunner, InputGradRunner
    dev = _dev()
    n = 2
    m = _build(dev).eval()
    x = param_fill.make_input(n, 256, 51).to(dev)
    y = param_fill.make_labels(n).to(dev)
    ig = InputGradRunner(m, n, 256, precision="fp16")
    at = AttackRunner(m, n, 256, norm="linf", eps=EPS2, steps=2, precision="fp16")
    for r in (ig, at):
        r(x, y)
    g0, a0 = ig(x, y).clone(), at(x, y).clone()
    assert ig.graph is not None and at.graph is not None
    torch.manual_seed(5)
    params = [p for p in m.parameters() if p.requires_grad]
    for p in params:
        p.grad = torch.randn_like(p) * 1e-2
    opt = torch.optim.AdamW(params, lr=1e-3)
    ptrs = [p.data_ptr() for p in params]
    opt.step()
    assert ptrs == [p.data_ptr() for p in params]
    m.zero_grad(set_to_none=True)
    for blk in (m.backbone._blocks[3], m.backbone._blocks[12]):               # an expanding block and a spectral block
        blk._bn0.running_mean.add_(0.05)
        blk._bn1.running_var.mul_(1.5)
        blk._bn2.running_var.mul_(1.2)
    m.backbone._bn0.running_mean.add_(0.02)                                   # the stem's, applied by block 0's kernels
    g1, a1 = ig(x, y).clone(), at(x, y).clone()
    assert _rl2(g1, g0) > 1e-2                                                # the step changed the function
    ig2 = InputGradRunner(m, n, 256, precision="fp16")
    at2 = AttackRunner(m, n, 256, norm="linf", eps=EPS2, steps=2, precision="fp16")
    for r in (ig2, at2):
        r(x, y)
    assert torch.equal(g1, ig2(x, y))
    assert torch.equal(a1, at2(x, y))
    assert not torch.equal(a1, a0)


def test_fp16_runner_cache_on_the_model():
    dev = _dev()
    m = _build(dev).eval()
    r32 = m.input_grad_runner(2, 256)
    r16 = m.input_grad_runner(2, 256, precision="fp16")
    assert r16 is not r32 and r16.half and not r32.half
    assert m.input_grad_runner(2, 256, precision="fp16", grad_scale=1024) is r16
    assert m.input_grad_runner(2, 256) is r32
    a16 = m.attack_runner(2, 256, eps=EPS2, steps=2, precision="fp16")
    assert m.attack_runner(2, 256, eps=EPS2, steps=2, precision="fp16") is a16
    assert m.attack_runner(2, 256, eps=EPS2, steps=2) is not a16
    for i in range(6):
        m.input_grad_runner(i + 3, 256, precision="fp16")
    assert len(m._ud_grad_runners) == 4


# ---- 6. the engine ------------------------------------------------------------------------------------------------------------
def test_engine_test_robust_fp16():
    _dev()
    from tests.test_d_train_engine import CONFIG
    from unidefense_amd.engine import get_engine
    torch.manual_seed(0)
    eng = get_engine("FE")(copy.deepcopy(CONFIG), "Test")
    # the engine's freshly initialised UDEB4 scores every input 0.5 exactly (nothing for an attack to move): the suite's filled model
    param_fill.fill_module_(eng.model_without_ddp, sf_coef=0.0, fuse_coef=0.3)
    res = eng.test_robust(batches=2, attack={"norm": "linf", "eps": EPS2, "steps": 2, "precision": "fp16"})
    assert set(res) == {"clean", "adv", "attack"}
    assert res["attack"]["precision"] == "fp16" and res["attack"]["grad_scale"] == 1024.0 and res["attack"]["steps"] == 2
    assert torch.isfinite(res["adv"]["scores"]).all() and torch.equal(res["adv"]["labels"], res["clean"]["labels"])
    assert not torch.equal(res["adv"]["scores"], res["clean"]["scores"])

    def mean_ce(r):
        p, lb = r["scores"].double(), r["labels"]
        return float(-torch.log(torch.where(lb == 0, p, 1.0 - p).clamp_min(1e-30)).mean())
    clean, adv = mean_ce(res["clean"]), mean_ce(res["adv"])
    print(f"  mean cross-entropy of the scores: clean {clean:.6f}  adv (fp16 attack) {adv:.6f}")
    assert adv > clean
    r32 = eng.test_robust(batches=2, attack={"norm": "linf", "eps": EPS2, "steps": 2})
    assert r32["attack"]["precision"] == "fp32" and r32["attack"]["grad_scale"] == 1.0
    assert torch.equal(r32["clean"]["scores"], res["clean"]["scores"])
    z = eng.test_robust(batches=2, attack={"norm": "linf", "eps": 0.0, "steps": 2, "precision": "fp16", "grad_scale": 4096})
    assert z["attack"]["grad_scale"] == 4096.0
    assert torch.equal(z["adv"]["scores"], z["clean"]["scores"])              # eps = 0: x_adv is x, bitwise
    assert all(p.grad is None for p in eng.model_without_ddp.parameters())
