"""CPU: the C-ABI library loads and exports every symbol include/unidefense_hip.h declares, the ctypes
binding (unidefense_amd/lib.py) covers the same set, and the product fails loudly without a GPU."""
import ctypes
import functools
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "unidefense_hip.h")


@functools.lru_cache(None)
def header():
    """The header as unidefense_amd.lib's reader sees it, read afresh from the file: (protos, structs, consts).  The one reader
    of the header in the suite."""
    from unidefense_amd import lib
    with open(HEADER) as f:
        return lib.read_header(f.read())


def test_header_symbols_exported_and_bound():
    from unidefense_amd import lib
    names = sorted(header().protos)
    assert len(names) >= 38
    handle = ctypes.CDLL(lib.LIB_PATH)
    missing = [n for n in names if not hasattr(handle, n)]
    assert not missing, f"declared in the header but not exported: {missing}"
    assert sorted(lib.EXPORTED) == names, (set(lib.EXPORTED) ^ set(names))
    lib.load()


def test_binding_follows_every_prototype():
    """argtypes and restype of every loaded function are the header's; no `ud_...(` of the header is left out"""
    from unidefense_amd import lib
    h, L = header(), lib.load()
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert len(re.findall(r"\bud_\w+\s*\(", text)) == len(h.protos) == len(lib.EXPORTED)
    assert tuple(h.protos) == lib.EXPORTED
    for name, (restype, params) in h.protos.items():
        fn = getattr(L, name)
        assert len(fn.argtypes) == len(params) and fn.restype is restype, name
        want = ctypes.c_long if re.search(rf"\blong\s+{name}\s*\(", text) else ctypes.c_int
        assert restype is want, name
        for t, (pt, pname) in zip(fn.argtypes, params):                 # struct classes are made per reading: compare by shape
            assert t is pt or (t.__name__ == pt.__name__ and ctypes.sizeof(t) == ctypes.sizeof(pt)), (name, pname)
    assert sum(r is ctypes.c_long for r, _ in h.protos.values()) == 18
    # spot checks against the header's text, one of each kind of parameter
    assert h.protos["ud_adamw_multi"][1][6:9] == [(ctypes.c_double, "beta1"), (ctypes.c_double, "beta2"), (ctypes.c_double, "eps")]
    assert [t for t, _ in h.protos["ud_sample_sumsq_ws_bytes"][1]] == [ctypes.c_int, ctypes.c_long]
    assert h.protos["ud_gemm_get_path"][1] == []
    assert h.protos["ud_gemm"][1][0] == (ctypes.POINTER(h.structs["ud_gemm_desc"]), "d")
    assert h.protos["ud_xchg_allreduce"][1][2] == (ctypes.c_void_p, "peers")
    assert h.consts["UD_EINVAL"] == -1000 and lib.const("UD_EINVAL") == -1000 and lib.const("UD_APGD_MAX_CHECKPOINTS") == 16
    for py, td in (("ConvGeom", "ud_conv_geom"), ("GemmDesc", "ud_gemm_desc"), ("GemmP3Desc", "ud_gemm_p3_desc"),
                   ("SplitItem", "ud_split_item"), ("LayoutItem", "ud_layout_item"), ("BnRef", "ud_bn_ref"),
                   ("LossTail", "ud_loss_tail"), ("WgradFold", "ud_wgrad_fold")):
        assert [n for n, _ in getattr(lib, py)._fields_] == [n for n, _ in h.structs[td]._fields_], py
    assert set(h.structs) == {"ud_conv_geom", "ud_gemm_desc", "ud_gemm_p3_desc", "ud_split_item", "ud_layout_item", "ud_bn_ref",
                              "ud_loss_tail", "ud_wgrad_fold"}


def test_row_tables_derived_from_the_header_keep_their_keys_and_values():
    """the tables no family test states literally (the FMN, sparse FMN, Square, warp and spatial ones are in their own files)"""
    from unidefense_amd import kernels as K
    assert K.APGD_MAX_CHECKPOINTS == 16
    assert K.APGD_I == {"k": 0, "cnt": 1, "halved": 2, "improved": 3, "reset": 4}
    assert K.APGD_F == {"f_prev": 0, "f_best": 1, "f_ckpt": 2, "eta": 3, "a": 4}
    assert K.CORRUPT_JPEG == {"420": 0, "444": 1}
    assert K.CORRUPT_POINT == {"contrast": 0, "saturation": 1, "gaussian_noise": 2}


def test_struct_layouts_match_the_compiler(tmp_path):
    """sizeof and every offsetof of the header's structs, printed by a host-only C program built with the Makefile's compiler,
    against the ctypes classes derived from the same header"""
    from unidefense_amd import lib
    structs = header().structs
    with open(os.path.join(ROOT, "unidefense_amd", "csrc", "Makefile")) as f:
        hipcc = re.search(r"^HIPCC\s*[?:]?=\s*(\S+)", f.read(), flags=re.M).group(1)
    hipcc = os.environ.get("HIPCC", hipcc)
    lines = ["#include <stddef.h>", "#include <stdio.h>", f'#include "{HEADER}"', "int main(void) {"]
    for td, cls in structs.items():
        lines.append(f'    printf("{td} %zu\\n", sizeof({td}));')
        lines += [f'    printf("{td}.{n} %zu\\n", offsetof({td}, {n}));' for n, _ in cls._fields_]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    r = subprocess.run([hipcc, "-x", "c", str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=30, check=True).stdout
    got = {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}
    want = {}
    for py, td in (("ConvGeom", "ud_conv_geom"), ("GemmDesc", "ud_gemm_desc"), ("GemmP3Desc", "ud_gemm_p3_desc"),
                   ("SplitItem", "ud_split_item"), ("LayoutItem", "ud_layout_item"), ("BnRef", "ud_bn_ref"),
                   ("LossTail", "ud_loss_tail"), ("WgradFold", "ud_wgrad_fold")):
        cls = getattr(lib, py)                              # the classes the product uses, not the test's own reading
        want[td] = ctypes.sizeof(cls)
        want.update({f"{td}.{n}": getattr(cls, n).offset for n, _ in cls._fields_})
    assert len(structs) == 8 and got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}


GOOD = """
/* a comment with int ud_not_this(int x); inside */
#ifndef T_H
#define T_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define UD_NEG (-7)
#define UD_ROW_A 0
#define UD_ROW_B_C 1
#define UD_TEXT 1 << 4
typedef void* ud_stream_t;
typedef struct { int a, b[2]; const float* p; float* q; double d; } ud_inner;
typedef struct {
    const uint16_t* A; long n;     /* two on a line */
    ud_inner g;
    void* feat[3];
} ud_outer;
int ud_f(const ud_outer* o, const ud_inner* i, unsigned char* m, void* const* pp, long n, float x, double y,
         ud_stream_t
         stream);
long ud_g(void);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_reader_round_trips_a_well_formed_header():
    from unidefense_amd import lib
    h = lib.read_header(GOOD)
    c = ctypes
    inner, outer = h.structs["ud_inner"], h.structs["ud_outer"]
    assert list(h.structs) == ["ud_inner", "ud_outer"] and list(h.protos) == ["ud_f", "ud_g"]
    assert inner._fields_ == [("a", c.c_int), ("b", c.c_int * 2), ("p", c.c_void_p), ("q", c.c_void_p), ("d", c.c_double)]
    assert outer._fields_ == [("A", c.c_void_p), ("n", c.c_long), ("g", inner), ("feat", c.c_void_p * 3)]
    assert h.protos["ud_g"] == (c.c_long, [])
    assert h.protos["ud_f"] == (c.c_int, [(c.POINTER(outer), "o"), (c.POINTER(inner), "i"), (c.c_void_p, "m"), (c.c_void_p, "pp"),
                                           (c.c_long, "n"), (c.c_float, "x"), (c.c_double, "y"), (c.c_void_p, "stream")])
    assert h.consts == {"UD_NEG": -7, "UD_ROW_A": 0, "UD_ROW_B_C": 1, "UD_TEXT": "1 << 4"}
    assert lib.const("UD_NEG", h.consts) == -7
    with pytest.raises(lib.UDLibraryError, match="UD_TEXT.*1 << 4"):          # no integer: refused when asked for
        lib.const("UD_TEXT", h.consts)
    with pytest.raises(lib.UDLibraryError, match="UD_MISSING"):
        lib.const("UD_MISSING", h.consts)


@pytest.mark.parametrize("text,quote", [
    ("int ud_f(size_t n);", "size_t n"),                                          # an unknown type
    ("int ud_f(short* p);", "short"),                                             # ... behind a pointer too
    ("int ud_f(int n", "ud_f"),                                                   # an unterminated prototype
    ("int ud_f(int n\nint ud_g(int m);", "ud_f"),                                 # ... with another behind it
    ("int ud_f(const ud_thing* t);\ntypedef struct { int a; } ud_thing;", "ud_thing"),     # a struct used before it is declared
    ("typedef struct { ud_later g; } ud_now;", "ud_later"),
    ("typedef void* ud_stream_t;\nint ud_f(ud_stream_t* s);", "ud_stream_t"),     # declarator shapes outside the dialect
    ("int ud_f(int (*cb)(int));", "ud_f"),
    ("int ud_f(int);", "int"),
    ("typedef struct { int* a, b; } ud_s;", "int* a, b"),
    ("typedef struct { int a : 3; } ud_s;", "a : 3"),
    ("float ud_f(int n);", "ud_f"),                                               # a ud_...( that is no int / long prototype
    ("static inline int ud_f(int n) { return n; }", "ud_f"),
    ("void ud_f(int n);", "ud_f"),
    ("#if UD_X\nint ud_f(int n);\n#endif", "#if UD_X"),                           # preprocessor forms outside the dialect
    ("#define UD_F(x) (x)", "UD_F"),
    ("#define OTHER 3", "OTHER"),
    ("#pragma once", "pragma"),
])
def test_reader_refuses_what_it_does_not_know(text, quote):
    from unidefense_amd import lib
    with pytest.raises(lib.UDLibraryError) as e:
        lib.read_header(text)
    assert quote in str(e.value), str(e.value)


def test_invalid_arguments_are_rejected_without_gpu():
    from unidefense_amd import lib
    # argument validation happens before any HIP call
    assert lib.load().ud_gemm(None, None) == -1000
    assert lib.load().ud_reduce_ws_doubles(0, 16, 8) == -1000      # G < 1
    assert lib.load().ud_rfft2(None, None, 1, 14, 4, 1.0, 1.0, 0, None) == -1000   # no in-register transform for this side (kernels.py falls back to DFT matrices)
    assert lib.load().ud_rfft2(None, None, 1, 20, 4, 1.0, 1.0, 1, None) == -1000   # 5*2^k sizes: fp32 storage only
    with pytest.raises(lib.UDLibraryError):
        lib.call("ud_reduce_ws_doubles", 0, 16, 8)


def test_model_refuses_cpu_tensors():
    from unidefense_amd.model import load_model
    m = load_model("udeb4")(extractor="efficientnet-b4", num_classes=2)
    with pytest.raises(RuntimeError, match="GPU only"):
        m.eval()(torch.zeros(1, 3, 256, 256))


def test_state_dict_keys_match_reference_layout():
    """802 keys / 505 parameters / 128.3 M values with the reference's names."""
    from oracle import eb4
    from unidefense_amd.model import load_model
    m = load_model("UDEB4")(extractor="efficientnet-b4", num_classes=2, drop_rate=0.5)
    sd = m.state_dict()
    want = eb4.eb4_state_shapes(2)
    assert set(sd) == set(want)
    assert all(tuple(sd[k].shape) == tuple(want[k]) for k in want)
    assert len(list(m.parameters())) == 505
    assert not m.bottleneck.bias.requires_grad


def test_dropin_shims_resolve_the_reference_import_names():
    """`from engine import get_engine`, `from model import load_model`, `from loss import get_loss`
    (main.py:5-6 and the engines of the reference) with unidefense_amd/dropin first on sys.path — in a fresh interpreter."""
    import subprocess
    import sys
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from engine import get_engine\nfrom model import load_model\nfrom loss import get_loss\n"
            "import unidefense_amd.engine as e, unidefense_amd.model as m\n"
            "assert get_engine is e.get_engine and load_model is m.load_model\n"
            "assert get_engine('UE').__name__ == 'TrainEngine' and load_model('udr50').__name__ == 'UniDefenseModelRes50'\n"
            "print('ok')" % (os.path.join(ROOT, "unidefense_amd", "dropin"), ROOT))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/tmp", timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-1500:]
