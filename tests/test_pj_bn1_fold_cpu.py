"""No GPU: the host side of the thin-project blocks' BatchNorm-1 fold — the entry points are declared, exported and refuse
what they do not take before any launch; the routing policy and its override."""
import ctypes

import torch

ENTRIES = ("ud_pj_bwd_fused_se_ok", "ud_pj_bwd_fused_a_se", "ud_pj_bwd_fused_c", "ud_pj_bwd_fused_c_mix")
EINVAL = -1000


def test_entry_points_are_declared_and_exported():
    from unidefense_amd import lib
    h = lib.load()
    for name in ENTRIES:
        assert name in lib.EXPORTED and hasattr(h, name), name
    # the pairs built: those of ud_pj_bwd_fused_ok but the 24-column ones; whole 32-row tiles per sample
    for ce, co in ((144, 32), (192, 32), (336, 56), (192, 56)):
        assert h.ud_pj_bwd_fused_se_ok(ce, co, 64) == 1 and h.ud_pj_bwd_fused_se_ok(ce, co, 48) == 0
    for ce, co in ((48, 24), (24, 24)):
        assert h.ud_pj_bwd_fused_ok(ce, co, 64) == 1 and h.ud_pj_bwd_fused_se_ok(ce, co, 64) == 0
    assert h.ud_pj_bwd_fused_se_ok(64, 16, 64) == 0


def test_entry_points_refuse_eval_form_null_tensors_and_unbuilt_pairs():
    from unidefense_amd import kernels as K, lib
    h = lib.load()
    N, HW, CE, CO = 2, 64, 192, 32
    mod = torch.nn.BatchNorm2d(CE).eval()
    ev = ctypes.byref(K.EvalBN(mod, 1).ref())
    acc = torch.zeros(2 * CE, dtype=torch.float64)
    tr = ctypes.byref(K.DeferredBN(acc, CE, N * HW, mod.weight, mod.bias, 1e-3, 1).ref())
    d = torch.zeros(N, HW, CE)
    dp = torch.zeros(N * HW, CO)
    s = torch.zeros(N, CE)
    w = torch.zeros(CO, CE)
    dots = torch.zeros(5 * N * CE, dtype=torch.float64)
    part = torch.zeros(512 * CO * CE)
    p, pd = K._p, K._pd

    def a_se(bn=tr, hw=HW, ce=CE, co=CO, **nul):
        t = dict(d=p(d), dp=p(dp), s=p(s), w=p(w), dw=p(w), dots=pd(dots), part=p(part))
        t.update(nul)
        return h.ud_pj_bwd_fused_a_se(t["d"], t["dp"], bn, t["s"], t["w"], N, hw, ce, co, t["dw"], t["dots"], t["part"], None)

    def c_args(nul):
        t = dict(d=p(d), dp=p(dp), s=p(s), dpool=p(s), w=p(w), s1=pd(acc), s2=pd(acc, CE), s1l=pd(acc), s2l=pd(acc, CE), dd=p(d),
                 dg=None, db=None, diff=p(d), dacc=pd(dots))
        t.update(nul)
        return t

    def c(bn=tr, hw=HW, ce=CE, co=CO, **nul):
        t = c_args(nul)
        return h.ud_pj_bwd_fused_c(t["d"], t["dp"], bn, t["s"], t["dpool"], 1.0 / HW, t["w"], t["s1"], t["s2"], t["s1l"], t["s2l"], N, hw,
                                   ce, co, t["dd"], t["dg"], t["db"], None)

    def c_mix(bn=tr, hw=HW, ce=CE, co=CO, **nul):
        t = c_args(nul)
        return h.ud_pj_bwd_fused_c_mix(t["d"], t["dp"], bn, t["s"], t["dpool"], 1.0 / HW, t["w"], t["s1"], t["s2"], t["s1l"], t["s2l"],
                                       t["diff"], N, hw, ce, co, t["dd"], t["dacc"], t["dg"], t["db"], None, None)

    for f in (a_se, c, c_mix):
        assert f(bn=ev) == EINVAL          # a training-form backward: the eval form is refused
        assert f(bn=None) == EINVAL
        assert f(hw=48) == EINVAL          # HW % 32
        assert f(ce=64, co=16) == EINVAL          # a pair that is not built
        assert f(ce=48, co=24) == EINVAL          # ... and the narrow pairs, which keep passes A and B
        for name in ("d", "dp", "s", "w"):
            assert f(**{name: None}) == EINVAL, name
    for name in ("dw", "dots", "part"):
        assert a_se(**{name: None}) == EINVAL, name
    for f in (c, c_mix):
        for name in ("dpool", "s1", "s2", "dd"):
            assert f(**{name: None}) == EINVAL, name
        # dgamma / dbeta come from this rank's sums: asked for without them is refused
        assert f(dg=p(s), s2l=None) == EINVAL and f(db=p(s), s1l=None) == EINVAL
    assert c_mix(diff=None) == EINVAL and c_mix(dacc=None) == EINVAL


def test_policy_rule_and_override(monkeypatch):
    from unidefense_amd import mbconv as MB
    assert not MB._PJ_BN1_FOLD_OVERRIDE
    for key, rule in MB._PJ_BN1_FOLD_RULE.items():
        assert MB._pj_bn1_fold_policy(*key) is rule
    # the eight thin-project blocks of UDEB4 at 256 x 256 are the table's keys; a shape outside it keeps passes A and B
    assert set(MB._PJ_BN1_FOLD_RULE) == {(False, 2, 64, 144), (False, 1, 64, 192), (True, 2, 32, 192), (True, 1, 32, 336)}
    assert MB._pj_bn1_fold_policy(False, 1, 8, 192) is False
    key = (True, 1, 32, 336)
    for ov in (False, True):
        monkeypatch.setitem(MB._PJ_BN1_FOLD_OVERRIDE, key, ov)
        assert MB._pj_bn1_fold_policy(*key) is ov
        assert MB._pj_bn1_fold_policy(1, 1, 32, 336) is ov          # keys are normalised to bool
    monkeypatch.setitem(MB._PJ_BN1_FOLD_OVERRIDE, (False, 1, 8, 192), True)
    assert MB._pj_bn1_fold_policy(False, 1, 8, 192) is True          # the override reaches a shape outside the table
    # the policy of the blocks with a dc tensor is a different one and stays as it was
    assert MB._se_bn1_fold_policy(False, 1, 64, 192, False) is True and not MB._SE_BN1_FOLD_OVERRIDE
