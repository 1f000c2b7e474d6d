"""CPU: the eval form of ud_bn_ref (kernels.EvalBN) and the argument checks of the eval-mode MBConv kernel (csrc/evalblk.hip),
which all run before any HIP call."""
import ctypes

import torch


def test_eval_bn_ref_is_the_eval_form():
    from unidefense_amd import kernels as K
    bn = torch.nn.BatchNorm2d(16, eps=1e-3).eval()
    r = K.EvalBN(bn, 1).ref(update=True)
    assert r.sum is None and r.sumsq is None
    assert r.running_mean == bn.running_mean.data_ptr() and r.running_var == bn.running_var.data_ptr()
    assert r.gamma == bn.weight.data_ptr() and r.beta == bn.bias.data_ptr()
    assert r.act == 1 and r.G == 1 and abs(r.eps - 1e-3) < 1e-9
    plain = K.EvalBN(torch.nn.BatchNorm2d(8, affine=False).eval(), 0).ref()
    assert plain.gamma and plain.beta and plain.act == 0


def test_mb_eval_dw_takes_the_udeb4_blocks():
    from unidefense_amd import kernels as K, lib
    for ci, ce, s in ((24, 144, 2), (32, 192, 1), (272, 1632, 1), (448, 2688, 1)):
        assert K.mb_eval_dw_ok(ci, ce, 3, s), (ci, ce, s)
    assert not K.mb_eval_dw_ok(32, 192, 5, 1)
    assert not K.mb_eval_dw_ok(30, 192, 3, 1)
    assert not K.mb_eval_dw_ok(32, 200, 3, 1)
    assert not K.mb_eval_dw_ok(32, 192, 3, 3)
    h = lib.load()
    assert h.ud_mb_eval_dw_tiles(64, 64, 1) == 8 * 4
    assert h.ud_mb_eval_dw_tiles(8, 8, 1) == 1
    assert h.ud_mb_eval_dw_tiles(95, 95, 2) == 12 * 12
    assert h.ud_mb_eval_dw_tiles(0, 8, 1) == -1000


def test_mb_eval_dw_and_backward_entries_refuse_bad_arguments():
    from unidefense_amd import kernels as K, lib
    h = lib.load()
    bn = torch.nn.BatchNorm2d(192).eval()
    ev = ctypes.byref(K.EvalBN(bn, 1).ref())
    # NULL tensors
    assert h.ud_mb_eval_dw(None, None, ev, None, ev, None, None, 1, 8, 8, 32, 192, 8, 8, 3, 1, 1, 1, 1, None) == -1000
    # a training-form BatchNorm (sum set) is not taken by the eval kernel
    acc = torch.zeros(2 * 192, dtype=torch.float64)
    tr = ctypes.byref(K.DeferredBN(acc, 192, 64, bn.weight, bn.bias, 1e-3, 1).ref())
    x = torch.zeros(1, 8, 8, 32)
    w = torch.zeros(192, 32)
    args = [K._p(x), K._p(w), None, K._p(w), None, K._p(w), K._p(w), 1, 8, 8, 32, 192, 8, 8, 3, 1, 1, 1, 1, None]
    args[2], args[4] = tr, ev
    assert h.ud_mb_eval_dw(*args) == -1000
    # backward entry points refuse the eval form before touching their tensors
    assert h.ud_coldot_bn(None, None, ev, 1, 64, 192, None, None, 0, None) == -1000
    assert h.ud_pw_bwd_fused(None, None, ev, None, None, None, None, None, None, None, 64, 192, 32, None, None, None, None,
                             None, None) == -1000
    assert h.ud_pj_bwd_fused_a(None, None, ev, None, None, 1, 64, 192, 32, None, None, None, None) == -1000
