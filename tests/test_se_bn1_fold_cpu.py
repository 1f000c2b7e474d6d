"""No GPU: the host side of the SE / BatchNorm-1 backward without dz1 — the four entry points are declared, exported and
refuse what they do not take before touching a tensor; the routing policy and its override."""
import ctypes

import torch

ENTRIES = ("ud_coldot_bn_se", "ud_se_bwd_b_bn", "ud_normbwd_apply_se", "ud_normbwd_apply_mix_se")


def test_entry_points_are_declared_and_exported():
    from unidefense_amd import lib
    h = lib.load()
    for name in ENTRIES:
        assert name in lib.EXPORTED and hasattr(h, name), name


def test_entry_points_refuse_eval_form_half_storage_and_null_tensors():
    from unidefense_amd import kernels as K, lib
    h = lib.load()
    C, G, R = 192, 2, 64
    bn = torch.nn.BatchNorm2d(C).eval()
    ev = ctypes.byref(K.EvalBN(bn, 1).ref())
    acc = torch.zeros(2 * C, dtype=torch.float64)
    tr = ctypes.byref(K.DeferredBN(acc, C, G * R, bn.weight, bn.bias, 1e-3, 1).ref())
    x = torch.zeros(G, R, C)
    s = torch.zeros(G, C)
    out = torch.zeros(5 * G * C, dtype=torch.float64)
    p, pd = K._p, K._pd

    def dot(b, f16=0, xx=x):
        return h.ud_coldot_bn_se(p(xx), p(xx), b, G, R, C, pd(out), f16, None)

    def apply(b, f16=0, dc=x):
        return h.ud_normbwd_apply_se(p(x), p(dc), b, p(s), p(s), 1.0 / R, pd(acc), pd(acc, C), pd(acc), pd(acc, C), G, R, C, p(x),
                                     None, None, f16, None, None)

    def mix(b, f16=0, diff=x):
        return h.ud_normbwd_apply_mix_se(p(x), p(x), b, p(s), p(s), 1.0 / R, pd(acc), pd(acc, C), pd(acc), pd(acc, C), p(diff), G, R,
                                         C, p(x), pd(out), None, None, None, f16, None)

    for f in (dot, apply, mix):
        assert f(ev) == -1000          # a training-form backward: the eval form is refused
        assert f(tr, 1) == -1000       # fp32 storage only
        assert f(tr, 0, None) == -1000          # a NULL tensor
    assert h.ud_coldot_bn_se(p(x), p(x), tr, G, R, 190, pd(out), 0, None) == -1000          # C % 4
    # ud_se_bwd_b's own checks, and the fold's operands
    d1 = torch.zeros(G * 8, dtype=torch.float64)
    w = torch.zeros(8, C)
    args = [pd(d1), p(torch.zeros(G, 8)), p(w), pd(out), 0.5, p(s), p(w), p(torch.zeros(8)), p(s), pd(out), 1.0 / R, pd(acc),
            pd(acc, C), G, C, 8, None]
    for i in (8, 9, 11, 12):          # s2, dots, bs1, bs2
        bad = list(args)
        bad[i] = None
        assert h.ud_se_bwd_b_bn(*bad) == -1000
    bad = list(args)
    bad[13] = 257          # N > 256, as ud_se_bwd_b
    assert h.ud_se_bwd_b_bn(*bad) == -1000


def test_policy_rule_and_override(monkeypatch):
    from unidefense_amd import mbconv as MB
    assert not MB._SE_BN1_FOLD_OVERRIDE
    for key in ((False, 1, 128, 48), (True, 2, 16, 336), (True, 1, 16, 672), (True, 1, 8, 1632), (False, 1, 8, 2688)):
        assert MB._se_bn1_fold_policy(*key, False) is True
        assert MB._se_bn1_fold_policy(*key, True) is False          # half storage keeps the old chain
    key = (True, 1, 16, 960)
    monkeypatch.setitem(MB._SE_BN1_FOLD_OVERRIDE, key, False)
    assert MB._se_bn1_fold_policy(*key, False) is False
    assert MB._se_bn1_fold_policy(1, 1, 16, 960, False) is False          # keys are normalised to bool
    assert MB._se_bn1_fold_policy(True, 1, 16, 672, False) is True        # another shape keeps the rule
    monkeypatch.setitem(MB._SE_BN1_FOLD_OVERRIDE, key, True)
    assert MB._se_bn1_fold_policy(*key, True) is False                   # an override never routes half storage
