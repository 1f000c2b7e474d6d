"""CPU: argument checks of the input-gradient entry points (csrc/inputgrad.hip).  They validate before any HIP call, so the
unsupported geometries are refused with UD_EINVAL on a box without a GPU."""
import ctypes

import pytest
import torch

UD_EINVAL = -1000


def _geom(N=2, H=256, Cin=3, k=3, stride=2, pad=0, transposed=0, Ho=None):
    from unidefense_amd.lib import ConvGeom
    g = ConvGeom()
    Ho = (H + 2 * pad - k) // stride + 1 if Ho is None else Ho
    g.N, g.Hin, g.Win, g.Cin, g.Hout, g.Wout = N, H, H, Cin, Ho, Ho
    g.KH, g.KW, g.stride, g.pad_t, g.pad_l, g.transposed = k, k, stride, pad, pad, transposed
    return g


def test_stem_dgrad_supported_table():
    from unidefense_amd import lib
    f = lib.load().ud_stem_dgrad_supported
    assert f(3, 48, 3, 3, 2) == 1           # UDEB4
    assert f(3, 64, 7, 7, 2) == 1           # UDR18 / UDR50
    for args in ((3, 64, 3, 3, 2), (3, 48, 7, 7, 2), (4, 48, 3, 3, 2), (3, 48, 3, 3, 1), (3, 48, 3, 5, 2), (3, 32, 3, 3, 2)):
        assert f(*args) == 0, args


@pytest.mark.parametrize("kw", [dict(Cin=4), dict(k=5), dict(stride=1), dict(transposed=1), dict(pad=3), dict(N=0),
                                dict(k=7, pad=7), dict(Ho=0)])
def test_stem_dgrad_rejects_other_geometries(kw):
    from unidefense_amd import lib
    k = kw.get("k", 3)
    co = 64 if k == 7 else 48
    g = _geom(**kw)
    buf = ctypes.c_void_p(16)               # never dereferenced: the checks come first
    assert lib.load().ud_stem_dgrad(ctypes.byref(g), buf, buf, buf, co, 0, None) == UD_EINVAL


def test_stem_dgrad_rejects_wrong_cout_and_null_buffers():
    from unidefense_amd import lib
    g = _geom()
    buf = ctypes.c_void_p(16)
    assert lib.load().ud_stem_dgrad(ctypes.byref(g), buf, buf, buf, 64, 0, None) == UD_EINVAL
    assert lib.load().ud_stem_dgrad(ctypes.byref(g), None, buf, buf, 48, 0, None) == UD_EINVAL
    assert lib.load().ud_stem_dgrad(None, buf, buf, buf, 48, 0, None) == UD_EINVAL


def test_attention_helpers_reject_bad_arguments():
    from unidefense_amd import lib
    h = lib.load()
    buf = ctypes.c_void_p(16)
    assert h.ud_absdiff_bwd(buf, buf, buf, None, None, 10, None) == UD_EINVAL      # neither output
    assert h.ud_absdiff_bwd(buf, buf, buf, buf, None, -1, None) == UD_EINVAL
    assert h.ud_outer(buf, buf, buf, 10, 0, None) == UD_EINVAL
    assert h.ud_outer(None, buf, buf, 10, 3, None) == UD_EINVAL


def test_wrapper_refuses_unsupported_stem():
    from unidefense_amd import kernels as K
    g = K.conv_geom(1, 64, 64, 3, 32, 32, 5, 5, 2, 2, 2, 0)
    with pytest.raises(ValueError, match="no stem data-gradient kernel"):
        K.stem_dgrad(torch.zeros(1, 32, 32, 48), torch.zeros(48, 3, 5, 5), g)
