"""CPU: the precision argument of the input-gradient / attack runners (unidefense_amd/attack.py) and the argument checks of the
frozen backward's entry points (csrc/fused.hip, csrc/dwtile.hip, csrc/misc.hip), which all run before any HIP call."""
import ctypes

import pytest
import torch

FROZEN_ENTRIES = ("ud_coldot_bn_eval", "ud_coldot_bn_eval_ws_doubles", "ud_se_scale_bwd_bn_eval", "ud_bn_eval_bwd",
                  "ud_dwtile_dgrad_eval", "ud_sfmix_pool_bwd")


def test_frozen_entry_points_are_declared_exported_and_bound():
    from tests.test_abi_cpu import header
    from unidefense_amd import lib
    names = header().protos
    handle = ctypes.CDLL(lib.LIB_PATH)
    for n in FROZEN_ENTRIES:
        assert n in names, f"{n} is not declared in include/unidefense_hip.h"
        assert n in lib.EXPORTED, f"{n} is not bound in lib.EXPORTED"
        assert hasattr(handle, n), f"{n} is not exported by the library"


def _refs(C=192, act=1):
    from unidefense_amd import kernels as K
    bn = torch.nn.BatchNorm2d(C).eval()
    ev = K.EvalBN(bn, act)
    acc = torch.zeros(2 * C, dtype=torch.float64)
    tr = K.DeferredBN(acc, C, 64, bn.weight, bn.bias, 1e-3, act)
    return bn, acc, ev, tr


def test_coldot_bn_eval_refusals():
    from unidefense_amd import kernels as K, lib
    h = lib.load()
    bn, acc, ev, tr = _refs()
    x = torch.zeros(64, 192)
    out = torch.zeros(192, dtype=torch.float64)
    p, pd = K._p, K._pd
    assert h.ud_coldot_bn_eval(None, None, ctypes.byref(ev.ref()), 1, 64, 192, None, None, 0, None) == -1000          # NULL tensors
    assert h.ud_coldot_bn_eval(p(x), p(x), ctypes.byref(tr.ref()), 1, 64, 192, pd(out), None, 0, None) == -1000       # training form
    assert h.ud_coldot_bn_eval(p(x), p(x), None, 1, 64, 192, pd(out), None, 0, None) == -1000                         # no BatchNorm
    assert h.ud_coldot_bn_eval(p(x), p(x), ctypes.byref(ev.ref()), 1, 64, 190, pd(out), None, 0, None) == -1000       # C % 4
    assert h.ud_coldot_bn_eval(p(x), p(x), ctypes.byref(ev.ref()), 0, 64, 192, pd(out), None, 0, None) == -1000       # G < 1
    # more than one row-chunk per sample needs the scratch of the partials (no atomics across workgroups)
    assert h.ud_coldot_bn_eval_ws_doubles(1, 64, 192) == 0
    need = h.ud_coldot_bn_eval_ws_doubles(2, 4096, 192)
    assert need > 0 and need % (2 * 192) == 0
    assert h.ud_coldot_bn_eval(p(x), p(x), ctypes.byref(ev.ref()), 2, 4096, 192, pd(out), None, 0, None) == -1000
    assert h.ud_coldot_bn_eval_ws_doubles(1, 64, 190) == -1000
    with pytest.raises(lib.UDLibraryError):
        lib.call("ud_coldot_bn_eval_ws_doubles", 0, 64, 192)


def test_se_scale_bwd_bn_eval_and_bn_eval_bwd_refusals():
    from unidefense_amd import kernels as K, lib
    h = lib.load()
    bn, acc, ev, tr = _refs()
    x = torch.zeros(64, 192)
    s = torch.zeros(1, 192)
    p = K._p
    e, t = ctypes.byref(ev.ref()), ctypes.byref(tr.ref())
    assert h.ud_se_scale_bwd_bn_eval(None, None, e, None, None, 1.0, None, 1, 64, 192, 0, None) == -1000
    assert h.ud_se_scale_bwd_bn_eval(p(x), p(x), t, p(s), p(s), 1.0, p(x), 1, 64, 192, 0, None) == -1000
    assert h.ud_se_scale_bwd_bn_eval(p(x), p(x), e, p(s), p(s), 1.0, p(x), 1, 64, 2, 0, None) == -1000
    assert h.ud_se_scale_bwd_bn_eval(p(x), p(x), e, p(s), p(s), 1.0, p(x), 1, 0, 192, 0, None) == -1000
    assert h.ud_bn_eval_bwd(None, None, e, None, 1, 64, 192, 0, None) == -1000
    assert h.ud_bn_eval_bwd(p(x), p(x), t, p(x), 1, 64, 192, 0, None) == -1000
    assert h.ud_bn_eval_bwd(p(x), p(x), e, p(x), 1, 64, 193, 0, None) == -1000
    assert h.ud_bn_eval_bwd(p(x), None, e, p(x), 1, 64, 192, 0, None) == -1000          # swish needs the BatchNorm's input
    assert h.ud_sfmix_pool_bwd(None, None, 1, 8, 8, 192, 0, None) == -1000
    assert h.ud_sfmix_pool_bwd(p(x), p(x), 1, 8, 8, 190, 0, None) == -1000
    assert h.ud_sfmix_pool_bwd(p(x), p(x), 1, 0, 8, 192, 0, None) == -1000


def test_dwtile_dgrad_eval_refusals():
    from unidefense_amd import kernels as K, lib
    h = lib.load()
    bn, acc, ev, tr = _refs()
    x = torch.zeros(1, 8, 8, 192)
    wt = torch.zeros(9, 192)
    a = torch.zeros(1)
    p = K._p
    e, t = ctypes.byref(ev.ref()), ctypes.byref(tr.ref())

    def call(dy=x, w=wt, ga=None, gm=0, add=None, xb=x, ref=e, dx=x, N=1, H=8, W=8, C=192, Ho=8, Wo=8, k=3, pt=1, pl=1, s=1):
        return h.ud_dwtile_dgrad_eval(p(dy), p(w), p(ga), gm, p(add), p(xb), ref, p(dx), N, H, W, C, Ho, Wo, k, pt, pl, s, 0, None)
    assert call(dy=None) == -1000 and call(w=None) == -1000 and call(xb=None) == -1000 and call(dx=None) == -1000
    assert call(ref=t) == -1000                                   # a training-form BatchNorm
    assert call(ref=None) == -1000                                # the plain data gradient is ud_dwtile's (epi 2)
    assert call(k=4) == -1000 and call(s=3) == -1000 and call(C=190) == -1000 and call(pt=3) == -1000
    assert call(gm=1) == -1000 and call(gm=3, ga=a) == -1000      # a gate mode without its scalar / an unknown one
    assert call(Ho=40) == -1000 and call(H=64, W=64) == -1000     # extents no k x k conv of this stride relates


def _models():
    from unidefense_amd.model import load_model
    return {n: load_model(n)(num_classes=2, **(dict(extractor="efficientnet-b4") if n == "UDEB4" else {})).eval()
            for n in ("UDEB4", "UDR18", "UDR50")}


def test_runners_check_the_precision_before_cuda():
    from unidefense_amd.attack import AttackRunner, InputGradRunner, attack_runner, input_grad_runner
    ms = _models()
    for name, m in ms.items():
        makers = (lambda **kw: InputGradRunner(m, 2, 128, **kw), lambda **kw: AttackRunner(m, 2, 128, eps=0.01, **kw),
                  lambda **kw: input_grad_runner(m, 2, 128, **kw), lambda **kw: attack_runner(m, 2, 128, eps=0.01, **kw),
                  lambda **kw: m.input_grad_runner(2, 128, **kw), lambda **kw: m.attack_runner(2, 128, eps=0.01, **kw))
        for mk in makers:
            with pytest.raises(ValueError, match="precision must be one of"):
                mk(precision="bf16")
            if name == "UDEB4":
                with pytest.raises(ValueError, match="cuda"):          # a valid precision gets as far as the device check
                    mk(precision="fp16")
            else:
                with pytest.raises(ValueError, match=type(m).__name__):
                    mk(precision="fp16")
            with pytest.raises(ValueError, match="cuda"):
                mk(precision="fp32")
        assert not m.__dict__.get("_ud_grad_runners") and not m.__dict__.get("_ud_attack_runners")


def test_grad_scale_rules():
    from unidefense_amd.attack import DEFAULT_GRAD_SCALE, AttackRunner, InputGradRunner, resolve_grad_scale
    assert DEFAULT_GRAD_SCALE == 1024.0
    assert resolve_grad_scale("fp32", None) == 1.0 and resolve_grad_scale("fp32", 1) == 1.0
    assert resolve_grad_scale("fp16", None) == 1024.0
    assert resolve_grad_scale("fp16", 4096) == 4096.0 and resolve_grad_scale("fp16", 2.0 ** -3) == 0.125
    assert resolve_grad_scale("fp16", 1) == 1.0
    m = _models()["UDEB4"]
    for bad in (0, -1024.0, 1000.0, 3, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="power of two"):
            resolve_grad_scale("fp16", bad)
        with pytest.raises(ValueError, match="power of two"):
            InputGradRunner(m, 2, 256, precision="fp16", grad_scale=bad)
        with pytest.raises(ValueError, match="power of two"):
            AttackRunner(m, 2, 256, eps=0.01, precision="fp16", grad_scale=bad)
    for mk in (lambda **kw: InputGradRunner(m, 2, 256, **kw), lambda **kw: AttackRunner(m, 2, 256, eps=0.01, **kw),
               lambda **kw: m.input_grad_runner(2, 256, **kw), lambda **kw: m.attack_runner(2, 256, eps=0.01, **kw)):
        with pytest.raises(ValueError, match="fp32"):
            mk(grad_scale=1024.0)
        with pytest.raises(ValueError, match="fp32"):
            mk(precision="fp32", grad_scale=2)
        with pytest.raises(ValueError, match="cuda"):                  # None and 1 are taken
            mk(precision="fp32", grad_scale=1)


def test_cache_keys():
    from unidefense_amd.attack import attack_key, input_grad_key
    # the fp32 keys are what they were before the runners took a precision
    assert input_grad_key(2, 256) == (2, 256, "cross_entropy")
    assert input_grad_key(2, 256, "cross_entropy", "fp32", None) == input_grad_key(2, 256)
    assert input_grad_key(2, 256, precision="fp32", grad_scale=1) == input_grad_key(2, 256)
    old = (2, 256, "linf", 0.01, 10, None, False, False, (-1.0, 1.0), "cross_entropy")
    assert attack_key(2, 256, eps=0.01) == old
    assert attack_key(2, 256, eps=0.01, precision="fp32") == old
    # an fp16 runner has a key of its own, the default scale and the explicit one being the same runner
    k16 = input_grad_key(2, 256, precision="fp16")
    assert k16 != input_grad_key(2, 256) and k16 == input_grad_key(2, 256, precision="fp16", grad_scale=1024)
    assert k16 != input_grad_key(2, 256, precision="fp16", grad_scale=4096)
    a16 = attack_key(2, 256, eps=0.01, precision="fp16")
    assert a16 != old and a16[: len(old)] == old and a16 == attack_key(2, 256, eps=0.01, precision="fp16", grad_scale=1024.0)


def test_cache_limits_and_fp32_lookup_unchanged():
    from unidefense_amd import attack
    from unidefense_amd.infer import _MAX_RUNNERS
    assert _MAX_RUNNERS == 4

    class Owner:
        pass
    o = Owner()
    made = []
    for i in range(6):
        attack._cached(o, "_ud_grad_runners", attack.input_grad_key(i, 256, precision="fp16" if i % 2 else "fp32"),
                       lambda i=i: made.append(i) or i)
    assert len(o._ud_grad_runners) == 4 and made == list(range(6))
    assert attack._cached(o, "_ud_grad_runners", (4, 256, "cross_entropy"), lambda: "new") == 4          # the pre-existing fp32 key
