"""GPU, operator and block level: the SE / BatchNorm-1 backward whose BatchNorm sums come from per-sample dots and whose dz1 is
never written (csrc/fused.hip: ud_coldot_bn_se -> ud_se_bwd_b_bn -> ud_normbwd_apply_se / _mix_se) against torch in
float64 and against the chain it replaces (ud_coldot_bn -> ud_se_bwd_b -> ud_se_scale_bwd_bn -> ud_normbwd_apply[_mix]) on the same
inputs.

Shapes as in tests/test_b_bn_consumers_gpu.py (whose helpers are used): the row count R is chosen from the kernels' own
decomposition so that a thread of the geometry the case is about — 'redg' the per-group reduction of the dot kernel, 'ew' the
element-wise apply, 'mix' the SF-mix apply — walks exactly n rows, n = 1, 3, 4, 5, 11 (kRowGroup = 4); C = 8 / 36 / 144; G = 1 / 3;
act = swish and identity.  Bars: those tests/test_b_fused_kernels_gpu.py holds the same quantities to.

Observed on an MI355X (profiles/r23/se_bn1_fold.txt): see the table there."""
import ctypes

import pytest
import torch

from tests.test_b_bn_consumers_gpu import EPS, GC, NROWS, _act_grad, _bn, _dev, _inputs, _moments, _ref_fwd, _rel, _rows_for

pytestmark = pytest.mark.gpu

DGATE_TOL, SUM_TOL, DD_TOL = 5e-6, 1e-5, 2e-5
CS = 4          # squeeze width of the SE FCs in the operator cases


def _note(seen, name, v):
    """the worst figure of a quantity within one case (each case prints its own: -s shows them)"""
    seen[name] = max(seen.get(name, 0.0), float(v))


def _se_fc_inputs(G, C, g, dev):
    """what ud_se_bwd_b reads: ds1_acc fp64 [G][CS], s1 [G][CS], Wr [CS][C], the pooled sums fp64 [G][C]"""
    ds1 = torch.randn(G, CS, generator=g, device=dev).double()
    s1 = torch.randn(G, CS, generator=g, device=dev)
    Wr = torch.randn(CS, C, generator=g, device=dev) * 0.5
    pool = torch.randn(G, C, generator=g, device=dev).double()
    return ds1.contiguous(), s1, Wr, pool


def _se_bwd_b(K, ds1, s1, Wr, pool, G, C, fold=None):
    from unidefense_amd.lib import call
    dpool, dWr, dbr = torch.empty(G, C, device=s1.device), torch.empty(CS, C, device=s1.device), torch.empty(CS, device=s1.device)
    st = K._stream()
    if fold is None:
        call("ud_se_bwd_b", K._pd(ds1), K._p(s1), K._p(Wr), K._pd(pool), 0.25, K._p(dpool), K._p(dWr), K._p(dbr), G, C, CS, st)
    else:
        s2, dots, inv_hw, sacc = fold
        call("ud_se_bwd_b_bn", K._pd(ds1), K._p(s1), K._p(Wr), K._pd(pool), 0.25, K._p(dpool), K._p(dWr), K._p(dbr), K._p(s2),
             K._pd(dots), float(inv_hw), K._pd(sacc), K._pd(sacc, C), G, C, CS, st)
    return dpool, dWr, dbr


@pytest.mark.parametrize("kind", ["redg", "ew", "mix"])
@pytest.mark.parametrize("n", NROWS)
@pytest.mark.parametrize("G,C", GC)
def test_fold_chain_against_float64_and_the_old_chain(G, C, n, kind):
    from unidefense_amd import kernels as K
    dev = _dev()
    K.reset_zero_pool()
    R = _rows_for(n, kind, G, C)
    g, x, gamma, beta = _inputs(G, R, C, torch.float32, 29 * n + C + G + len(kind), dev)
    dc = torch.randn(G, R, C, generator=g, device=dev)
    s = torch.randn(G, C, generator=g, device=dev)
    diff = torch.randn(G, R, C, generator=g, device=dev)
    ds1, s1, Wr, pool = _se_fc_inputs(G, C, g, dev)
    cnt = G * R
    seen = {}
    k = gamma.double() / torch.sqrt(_moments(x)[2] + EPS)
    for act in (1, 0):
        a, z, xh = _ref_fwd(x, gamma, beta, act)
        bn = _bn(K, x, gamma, beta, act)
        # ---- the dot pass: dgate against float64 and against ud_coldot_bn
        dots = K.zeros64(5 * G * C, x)
        K.coldot_bn_se(dc, x, bn, G, R, dots)
        dgate_old = K.zeros64(G * C, x)
        K.coldot_bn(dc, x, bn, G, R, dgate_old)
        dgate = dots[:G * C]
        e = _rel(dgate.view(G, C), (dc.double() * a).sum(1))
        _note(seen, "dgate", e)
        assert e < DGATE_TOL
        assert _rel(dgate, dgate_old) < 1e-12          # (the same products, fp64 accumulation: the order of the adds is not fixed)
        # ---- the second SE FC: the same dpool / dWr / dbr, and the BatchNorm sums
        sacc = K.zeros64(2 * C, x)
        dpool, dWr, dbr = _se_bwd_b(K, ds1, s1, Wr, pool, G, C, fold=(s, dots, 1.0 / R, sacc))
        dpool_o, dWr_o, dbr_o = _se_bwd_b(K, ds1, s1, Wr, pool, G, C)
        assert torch.equal(dpool, dpool_o) and torch.equal(dWr, dWr_o) and torch.equal(dbr, dbr_o)
        dzr = (dc.double() * torch.sigmoid(s.double())[:, None, :] + dpool.double()[:, None, :] / R) * _act_grad(z, act)
        s1r, s2r = dzr.sum((0, 1)), (dzr * xh).sum((0, 1))
        e1, e2 = _rel(sacc[:C], s1r), _rel(sacc[C:], s2r)
        _note(seen, "s1", e1)
        _note(seen, "s2", e2)
        assert e1 < SUM_TOL and e2 < SUM_TOL
        ddr = k * (dzr - s1r / cnt - xh * s2r / cnt)
        terms = float((k * dzr).abs().max())
        # ---- the old chain on the same inputs
        sacc_o = K.zeros64(2 * C, x)
        dz_o = K.se_scale_bwd_bn(dc, x, bn, s, dpool, 1.0 / R, G, R, sacc_o)
        dd_o, _, _ = K.normbwd_apply(x, dz_o, None, 1.0, bn, True, G, R, sacc_o)
        # ---- the apply pass
        dd, dg, db = K.normbwd_apply_se(x, dc, bn, s, dpool, 1.0 / R, G, R, sacc)
        e_new, e_old = _rel(dd, ddr, terms), _rel(dd_o, ddr, terms)
        _note(seen, "dd", e_new)
        _note(seen, "dd (old chain)", e_old)
        assert e_new < DD_TOL
        assert e_new <= 2.0 * (e_old if e_old > 0.0 else 1e-6), (e_new, e_old)
        eg, eb = _rel(dg, s2r), _rel(db, s1r)
        _note(seen, "dgamma", eg)
        _note(seen, "dbeta", eb)
        assert eg < DD_TOL and eb < DD_TOL
        # ---- the SF-mix apply: dd, the gate's dot, the energy of dd
        for want_energy in (False, True):
            dacc, dacc_o = K.zeros64(64, x), K.zeros64(64, x)
            en = K.zeros64(C, x) if want_energy else None
            ddm, dgm, dbm = K.normbwd_apply_mix_se(x, dc, bn, s, dpool, 1.0 / R, G, R, sacc, diff, dacc, energy=en)
            ddm_o, _, _ = K.normbwd_apply_mix(x, dz_o, bn, G, R, sacc_o, diff, dacc_o)
            e_new, e_old = _rel(ddm, ddr, terms), _rel(ddm_o, ddr, terms)
            _note(seen, "dd (mix)", e_new)
            assert e_new < DD_TOL
            assert e_new <= 2.0 * (e_old if e_old > 0.0 else 1e-6), (e_new, e_old)
            assert _rel(dgm, s2r) < DD_TOL and _rel(dbm, s1r) < DD_TOL
            dot = ddm.double() * diff.double()
            edot = abs(float(dacc.sum()) - float(dot.sum())) / max(float(dot.abs().sum()), 1e-30)
            _note(seen, "sum dd diff", edot)
            assert edot <= DD_TOL
            dotr = ddr * diff.double()
            # (against float64 throughout: every element of dd is within DD_TOL * terms of the reference)
            assert abs(float(dacc.sum()) - float(dotr.sum())) <= DD_TOL * terms * float(diff.abs().sum())
            if want_energy:
                exact = ddm.double().pow(2).sum((0, 1))
                ok = exact > 0
                assert bool((en[~ok] == 0).all())
                if bool(ok.any()):          # (a batch of one row: dd = 0)
                    ratio = en[ok] / exact[ok]
                    _note(seen, "energy / exact - 1", float(ratio.max()) - 1.0)
                    assert float(ratio.min()) >= 1.0 and float(ratio.max()) < 1.001
    print(f"  G {G} C {C} n {n} {kind} (R {R}): " + ", ".join(f"{q} {v:.2e}" for q, v in seen.items()))


def test_eval_form_is_refused():
    """the new entry points are training-form backward entry points: an eval-form ud_bn_ref is UD_EINVAL"""
    from unidefense_amd import kernels as K
    from unidefense_amd import lib
    dev = _dev()
    K.reset_zero_pool()
    G, R, C = 2, 16, 8
    h = lib.load()
    einval = -1000
    mod = torch.nn.BatchNorm2d(C, eps=EPS).to(dev)
    x = torch.randn(G, R, C, device=dev)
    s = torch.randn(G, C, device=dev)
    dpool = torch.randn(G, C, device=dev)
    out, sacc, dacc = K.zeros64(5 * G * C, x), K.zeros64(2 * C, x), K.zeros64(64, x)
    dd = torch.empty_like(x)
    p, pd, st = K._p, K._pd, K._stream()
    ev = ctypes.byref(K.EvalBN(mod, 1).ref())
    assert h.ud_coldot_bn_se(p(x), p(x), ev, G, R, C, pd(out), 0, st) == einval
    assert h.ud_normbwd_apply_se(p(x), p(x), ev, p(s), p(dpool), 1.0 / R, pd(sacc), pd(sacc, C), pd(sacc), pd(sacc, C), G, R, C,
                                 p(dd), None, None, 0, None, st) == einval
    assert h.ud_normbwd_apply_mix_se(p(x), p(x), ev, p(s), p(dpool), 1.0 / R, pd(sacc), pd(sacc, C), pd(sacc), pd(sacc, C), p(x),
                                     G, R, C, p(dd), pd(dacc), None, None, None, 0, st) == einval
    # ... and half storage is not taken (fp32 storage only)
    tr = ctypes.byref(_bn(K, x, torch.ones(C, device=dev), torch.zeros(C, device=dev), 1).ref())
    assert h.ud_coldot_bn_se(p(x), p(x), tr, G, R, C, pd(out), 1, st) == einval
    assert h.ud_normbwd_apply_se(p(x), p(x), tr, p(s), p(dpool), 1.0 / R, pd(sacc), pd(sacc, C), pd(sacc), pd(sacc, C), G, R, C,
                                 p(dd), None, None, 1, None, st) == einval
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0          # nothing was launched


# ---------------------------------------------------------------------------------------------------------------------------
# block level: one fused MBConv training node of each kind, the policy forced on and forced off
def _block(kind, dev):
    from unidefense_amd.model.arch import BlockSpec
    from unidefense_amd.model.unidefense import _MBConvParams
    stride = 2 if kind == "sf2" else 1
    sp = BlockSpec(cin=16, cout=16 if stride == 1 else 24, cexp=64, expand=4, k=3, stride=stride,
                   pad=(1, 1, 1, 1) if stride == 1 else (0, 1, 0, 1), cse=4, sf_norm=None if kind == "plain" else "ortho",
                   skip=stride == 1)
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


def _run_block(blk, x, dout, keep):
    from unidefense_amd import kernels as K
    from unidefense_amd import mbconv as MB
    from unidefense_amd import tape as T
    K.begin_forward(blk)
    try:
        tape = T.Tape()
        w = blk._depthwise_conv.weight
        wts = K.dw_weights_tapmajor([w])
        T.DW_WT = {id(w): (w, w._version, wts[id(w)])}
        out = MB.mbconv_fused(tape, x, blk, keep, 0.8, wts[id(w)], T.DataParallelCtx(None, None))
    finally:
        K.end_forward()
    got = {}
    tape.nodes.insert(0, lambda: got.update(dx=tape.grads.get(id(x))))          # runs last in the reversed replay
    tape.add_grad(out, dout)
    K.reset_zero_pool()
    tape.backward()
    torch.cuda.synchronize()
    names = {id(p): k for k, p in blk.named_parameters()}
    return out, got["dx"], {names[id(p)]: g.clone() for p, g in tape.param_grads.items()}


@pytest.mark.parametrize("kind", ["plain", "sf1", "sf2"])
def test_block_gradients_agree_with_the_policy_on_and_off(kind, monkeypatch):
    from unidefense_amd import kernels as K
    from unidefense_amd import mbconv as MB
    dev = _dev()
    blk = _block(kind, dev)
    sp = blk.spec
    N, H = 2, 8 * sp.stride          # an 8 x 8 map behind the depthwise conv, 64 expanded channels
    g = torch.Generator(device=dev).manual_seed(41)
    x = torch.randn(N, H, H, sp.cin, generator=g, device=dev)
    dout = torch.randn(N, 8, 8, sp.cout, generator=g, device=dev)
    keep = torch.ones(N, device=dev) if sp.skip else None
    calls = {"se": 0, "old": 0}
    for name, slot in (("normbwd_apply_se", "se"), ("normbwd_apply_mix_se", "se"), ("se_scale_bwd_bn", "old")):
        def counted(*a, _f=getattr(K, name), _slot=slot, **kw):
            calls[_slot] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(K, name, counted)
    key = (sp.sf_norm is not None, sp.stride, 8, sp.cexp)
    res = {}
    for on in (True, False):
        monkeypatch.setitem(MB._SE_BN1_FOLD_OVERRIDE, key, on)
        res[on] = _run_block(blk, x, dout.clone(), keep)
    assert calls == {"se": 1, "old": 1}, calls          # each route ran once: the node does not take the thin-project kernels here
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
