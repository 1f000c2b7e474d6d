"""GPU, operator and block level: the thin-project blocks' BatchNorm-1 backward folded into the two passes over d (DESIGN 3z;
csrc/pjbwd.hip: ud_pj_bwd_fused_a_se -> ud_se_bwd_a, ud_se_bwd_b_bn -> ud_pj_bwd_fused_c / _c_mix; dz1 is never written) against
torch in float64 and against the chain it replaces (ud_pj_bwd_fused_a -> ud_pj_bwd_fused_b -> ud_normbwd_apply[_mix]) on the same
inputs.

Inputs: those of test_project_conv_backward_without_its_data_gradient (tests/test_b_fused_kernels_gpu.py), same generators.
Shapes (N, HW, Ce, Co, act): every built (Ce, Co) pair but the 24-column ones; a sample boundary inside a workgroup's tile range;
fewer tiles than workgroups and more (640 > 512; 192 > 170 per chunk of the 336-channel tensor); swish and identity.  The first
case carries a zero-gamma channel and a constant channel.  Bars: those of tests/test_b_se_bn1_fold_gpu.py and
tests/test_b_fused_kernels_gpu.py for the same quantities.

Observed on an MI355X: profiles/r28/pj_bn1_fold.txt, section 6."""
import pytest
import torch

from tests.test_b_bn_consumers_gpu import _act_grad, _dev, _rel
from tests.test_b_se_bn1_fold_gpu import DD_TOL, DGATE_TOL, SUM_TOL, _run_block, _se_bwd_b, _se_fc_inputs

pytestmark = pytest.mark.gpu

SHAPES = [(2, 64, 144, 32, 1), (3, 288, 192, 32, 1), (2, 96, 192, 32, 0), (2, 64, 336, 56, 1), (7, 160, 336, 56, 0),
          (3, 1024, 192, 56, 1), (5, 4096, 192, 32, 1), (6, 1024, 336, 56, 1)]


@pytest.mark.parametrize("N,HW,Ce,Co,act", SHAPES)
def test_fold_chain_against_float64_and_the_old_chain(N, HW, Ce, Co, act):
    from unidefense_amd import kernels as K
    dev = _dev()
    K.reset_zero_pool()
    g = torch.Generator().manual_seed(N * 7 + HW + Ce)
    M = N * HW
    d = (torch.randn(N, HW, Ce, generator=g) * 1.3 + 0.2)
    w = (torch.randn(Co, Ce, generator=g) / Ce ** 0.5).to(dev)
    dp = (torch.randn(M, Co, generator=g) * (0.3 + torch.rand(Co, generator=g))).to(dev)
    s = torch.randn(N, Ce, generator=g).to(dev)
    torch.randn(N, Ce, generator=g)          # (dpool there; here the second SE FC makes it)
    gamma, beta = (1.0 + 0.3 * torch.randn(Ce, generator=g)), (0.2 * torch.randn(Ce, generator=g))
    if (N, HW, Ce) == SHAPES[0][:3]:
        gamma[3] = 0.0          # a channel BatchNorm-1 scales to nothing
        d[:, :, 5] = 0.7        # a channel without variance
    d, gamma, beta = d.to(dev), gamma.to(dev), beta.to(dev)
    diff = torch.randn(N, HW, Ce, generator=torch.Generator(device=dev).manual_seed(HW + Ce), device=dev)
    acc = K.zeros64(2 * Ce, d)
    K.colstats(d.view(M, Ce), acc)
    bn = K.DeferredBN(acc, Ce, M, gamma, beta, 1e-3, act)
    assert K.project_bwd_fold_ok(w, HW)
    seen = {}

    def note(name, v):
        seen[name] = max(seen.get(name, 0.0), float(v))
        return v

    # ---- float64
    dd64 = d.double()
    mean, var = dd64.mean((0, 1)), dd64.var((0, 1), unbiased=False)
    inv = 1.0 / torch.sqrt(var + 1e-3)
    xh = (dd64 - mean) * inv
    z = gamma.double() * xh + beta.double()
    a = z * torch.sigmoid(z) if act else z
    da = _act_grad(z, act)
    dc64 = (dp.double() @ w.double()).view(N, HW, Ce)
    u64 = dc64 * da
    dots64 = torch.stack([(dc64 * a).sum(1), u64.sum(1), (u64 * xh).sum(1), da.sum(1), (da * xh).sum(1)])
    # ---- pass A: the weight gradient and the five dots; dgate and dWp are pass A's own
    dots = K.zeros64(5 * N * Ce, d)
    dw = K.project_bwd_fused_a_se(d, bn, s, dp, w, N, HW, dots)
    dgate_old = K.zeros64(N * Ce, d)
    dw_old = K.project_bwd_fused_a(d, bn, s, dp, w, N, HW, dgate_old)
    for i, name in enumerate(("dgate", "A1", "A2", "B1", "B2")):
        e = note(name, _rel(dots.view(5, N, Ce)[i], dots64[i]))
        assert e < DGATE_TOL, (name, e)
    e = note("dgate against pass A's", _rel(dots[:N * Ce], dgate_old))
    assert e <= 1e-12, e          # (the same products, the same fp32 tile sums: only the order of the fp64 adds is free)
    assert torch.equal(dw, dw_old)
    # ---- the second SE FC: dpool, and the BatchNorm sums from the dots
    gd = torch.Generator(device=dev).manual_seed(N + Ce)
    ds1, s1, Wr, pool = _se_fc_inputs(N, Ce, gd, dev)
    sacc = K.zeros64(2 * Ce, d)
    dpool, _, _ = _se_bwd_b(K, ds1, s1, Wr, pool, N, Ce, fold=(s, dots, 1.0 / HW, sacc))
    gate = torch.sigmoid(s.double()).view(N, 1, Ce)
    dz64 = (dc64 * gate + dpool.double().view(N, 1, Ce) / HW) * da
    s1r, s2r = dz64.sum((0, 1)), (dz64 * xh).sum((0, 1))
    e1, e2 = note("s1", _rel(sacc[:Ce], s1r)), note("s2", _rel(sacc[Ce:], s2r))
    assert e1 < SUM_TOL and e2 < SUM_TOL, (e1, e2)
    k = gamma.double() * inv
    ddr = k * (dz64 - s1r / M - xh * s2r / M)
    terms = float((k * dz64).abs().max())
    # ---- the old chain on the same inputs: pass B writes dz, the apply reads it
    sacc_o = K.zeros64(2 * Ce, d)
    dz_o = K.project_bwd_fused_b(d, bn, s, dpool, 1.0 / HW, dp, w, N, HW, sacc_o)
    dd_o, _, _ = K.normbwd_apply(d, dz_o, None, 1.0, bn, True, N, HW, sacc_o)
    # ---- pass C
    dd, dg, db = K.project_bwd_fused_c(d, bn, s, dpool, 1.0 / HW, dp, w, N, HW, sacc)
    e_new, e_old = note("dd", _rel(dd, ddr, terms)), note("dd (old chain)", _rel(dd_o, ddr, terms))
    assert e_new < DD_TOL
    assert e_new <= max(3e-6, 2.0 * e_old), (e_new, e_old)
    eg, eb = note("dgamma", _rel(dg, s2r)), note("dbeta", _rel(db, s1r))
    assert eg < DD_TOL and eb < DD_TOL
    # ---- pass C of the SF mix: dd, the gate's dot, the energy of dd
    for want_energy in (False, True):
        dacc, dacc_o = K.zeros64(64, d), K.zeros64(64, d)
        en = K.zeros64(Ce, d) if want_energy else None
        ddm, dgm, dbm = K.project_bwd_fused_c_mix(d, bn, s, dpool, 1.0 / HW, dp, w, N, HW, sacc, diff, dacc, energy=en)
        ddm_o, _, _ = K.normbwd_apply_mix(d, dz_o, bn, N, HW, sacc_o, diff, dacc_o)
        e_new, e_old = note("dd (mix)", _rel(ddm, ddr, terms)), _rel(ddm_o, ddr, terms)
        assert e_new < DD_TOL
        assert e_new <= max(3e-6, 2.0 * e_old), (e_new, e_old)
        assert _rel(dgm, s2r) < DD_TOL and _rel(dbm, s1r) < DD_TOL
        dot = ddm.double() * diff.double()
        edot = note("sum dd diff", abs(float(dacc.sum()) - float(dot.sum())) / max(float(dot.abs().sum()), 1e-30))
        assert edot <= DD_TOL
        # (against float64 throughout: every element of dd is within DD_TOL * terms of the reference)
        assert abs(float(dacc.sum()) - float((ddr * diff.double()).sum())) <= DD_TOL * terms * float(diff.abs().sum())
        if want_energy:
            exact = ddm.double().pow(2).sum((0, 1))
            ok = exact > 0
            assert bool((en[~ok] == 0).all())
            ratio = en[ok] / exact[ok]
            note("energy / exact - 1", float(ratio.max()) - 1.0)
            assert float(ratio.min()) >= 1.0 and float(ratio.max()) < 1.001, (float(ratio.min()), float(ratio.max()))
    print(f"  N {N} HW {HW} Ce {Ce} Co {Co} act {act}: " + ", ".join(f"{q} {v:.2e}" for q, v in seen.items()))


# ---------------------------------------------------------------------------------------------------------------------------
# block level: one fused MBConv training node whose geometry takes the thin-project kernels, the policy forced on and forced off
def _thin_block(kind, dev):
    from unidefense_amd.model.arch import BlockSpec
    from unidefense_amd.model.unidefense import _MBConvParams
    cin, cexp, cse = (32, 192, 8) if kind == "plain" else (56, 336, 14)
    sp = BlockSpec(cin=cin, cout=cin, cexp=cexp, expand=6, k=3, stride=1, pad=(1, 1, 1, 1), cse=cse,
                   sf_norm=None if kind == "plain" else "ortho", skip=True)
    torch.manual_seed(5)
    blk = _MBConvParams(sp, 1e-3, 0.01)
    with torch.no_grad():
        for name, prm in blk.named_parameters():
            if name.endswith("sf_coef"):
                prm.fill_(0.3)
            elif prm.dim() == 1:
                prm.copy_(1.0 + 0.2 * torch.randn_like(prm) if name.endswith("weight") else 0.1 * torch.randn_like(prm))
            else:
                prm.copy_(torch.randn_like(prm) * (2.0 / max(1, prm[0].numel())) ** 0.5)
    return blk.to(dev).train()


@pytest.mark.parametrize("kind", ["plain", "sf1"])
def test_block_gradients_agree_with_the_policy_on_and_off(kind, monkeypatch):
    from unidefense_amd import kernels as K
    from unidefense_amd import mbconv as MB
    dev = _dev()
    blk = _thin_block(kind, dev)
    sp = blk.spec
    N, H = 2, 8          # an 8 x 8 map: HW = 64, two tiles per sample
    g = torch.Generator(device=dev).manual_seed(41)
    x = torch.randn(N, H, H, sp.cin, generator=g, device=dev)
    dout = torch.randn(N, H, H, sp.cout, generator=g, device=dev)
    keep = torch.ones(N, device=dev)
    calls = {"new": 0, "old": 0}
    for name, slot in (("project_bwd_fused_c", "new"), ("project_bwd_fused_c_mix", "new"), ("project_bwd_fused_b", "old")):
        def counted(*a, _f=getattr(K, name), _slot=slot, **kw):
            calls[_slot] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(K, name, counted)
    key = (sp.sf_norm is not None, sp.stride, H, sp.cexp)
    res = {}
    for on in (True, False):
        monkeypatch.setitem(MB._PJ_BN1_FOLD_OVERRIDE, key, on)
        res[on] = _run_block(blk, x, dout.clone(), keep)
    assert calls == {"new": 1, "old": 1}, calls          # each route ran once: the node takes the thin-project kernels here
    (out1, dx1, pg1), (out0, dx0, pg0) = res[True], res[False]
    assert _rel(out1, out0) < 1e-6          # (the forward is the same code; its fp64 atomics add in no fixed order)
    assert set(pg1) == set(pg0) and {"_bn1.weight", "_bn1.bias", "_se_reduce.weight", "_project_conv.weight"} <= set(pg1)
    worst = _rel(dx1, dx0)
    assert worst <= 2e-5, ("dx", worst)
    for name in pg1:
        e = _rel(pg1[name], pg0[name])
        worst = max(worst, e)
        assert e <= 2e-5, (name, e)
    print(f"  block {kind}: policy on against off, worst relative difference {worst:.2e} over dx and {len(pg1)} parameter gradients")
