"""ctypes binding of libunidefense_hip.so, derived from the C ABI's own text (include/unidefense_hip.h).

The header is the only place where an entry point, a struct or a row constant is declared: read_header() turns its text into
prototypes, ctypes.Structure classes and the UD_* integers, and load() binds every prototype.  The reader accepts the header's
dialect and nothing else (INTEGRATION.md lists it); what it does not know raises UDLibraryError — it never guesses or skips.

The library is REQUIRED: load() without the built ``.so`` raises — there is no fallback path of any kind (no torch ops, no CPU
code) behind the product's operators.
"""
import collections
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
from .config import cfg as _cfg  # noqa: E402

LIB_PATH = _cfg.lib_path or os.path.join(_HERE, "libunidefense_hip.so")   # cfg.lib_path: A/B of kernel builds
HEADER_PATH = os.path.join(_HERE, "..", "include", "unidefense_hip.h")


class UDLibraryError(RuntimeError):
    pass


# ---- the header reader --------------------------------------------------------------------------------------------------------
Header = collections.namedtuple("Header", "protos structs consts")
# protos : name -> (restype, [(ctypes type, parameter name), ...]) in the header's order
# structs: typedef name -> ctypes.Structure class (its _fields_ are the header's fields, in order)
# consts : UD_NAME -> int (or the text of a value that is no integer literal: const() refuses it)

_SCALARS = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "double": C.c_double}
_POINTEES = set(_SCALARS) | {"void", "char", "unsigned char", "long long", "unsigned long long", "uint16_t", "uint32_t"}
_KEYWORDS = {"const", "struct", "unsigned", "signed", "short"} | {w for t in _POINTEES for w in t.split()}   # no parameter names
_ID = r"[A-Za-z_]\w*"
_DECL = re.compile(rf"(?P<base>{_ID}(?:\s+{_ID})*?)\s*(?P<stars>(?:\*\s*(?:const\b\s*)?)*)(?P<name>{_ID})\s*(?:\[(?P<n>\d+)\])?")
_MORE = re.compile(rf"(?P<name>{_ID})\s*(?:\[(?P<n>\d+)\])?")          # a further declarator of `int M, N, K;`
_STMT = re.compile(r"\s*(?:typedef\s+struct\s*\{(?P<body>[^{}]*)\}\s*(?P<struct>\w+)|(?P<plain>[^;{}]+?))\s*;")
_PROTO = re.compile(r"(?P<ret>int|long)\s+(?P<name>ud_\w+)\s*\((?P<args>[^()]*)\)")
_HANDLE = re.compile(rf"typedef\s+void\s*\*\s*(?P<name>{_ID})")
_DEFINE = re.compile(r"#\s*define\s+(?P<name>\w+)(?:\s+(?P<value>\S.*?))?\s*")
_IGNORED = re.compile(r"#\s*(?:ifndef\s+\w+|endif|include\s*<[\w./]+>)\s*")


def _refuse(why, decl):
    raise UDLibraryError(f"include/unidefense_hip.h: {why}: `{' '.join(decl.split())}`")


def read_header(text):
    """Header(protos, structs, consts) of a C header's text; UDLibraryError, quoting the declaration, for anything outside the
    dialect: an unknown type, declarator or preprocessor form, or a file-scope statement that is no prototype."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#\s*ifdef\s+__cplusplus\b.*?^[ \t]*#\s*endif[ \t]*$", "", text, flags=re.S | re.M)   # extern "C" { }
    protos, structs, handles, consts, code = {}, {}, set(), {}, []
    for line in text.split("\n"):
        if not line.lstrip().startswith("#"):
            code.append(line)
            continue
        line = line.strip()
        m = _DEFINE.fullmatch(line)
        if m and (m["value"] is None or m["name"].startswith("UD_")) and not line.endswith("\\"):
            if m["value"] is not None:
                v = m["value"]
                v = v[1:-1].strip() if v.startswith("(") and v.endswith(")") else v
                consts[m["name"]] = int(v) if re.fullmatch(r"-?\d+", v) else m["value"]
        elif not _IGNORED.fullmatch(line):
            _refuse("unknown preprocessor form", line)

    def ctype(decl, base, stars):
        base = " ".join(w for w in base.split() if w != "const")
        if base in structs or base in handles:
            if stars > (base in structs):
                _refuse("unknown declarator", decl)
            return C.c_void_p if base in handles else C.POINTER(structs[base]) if stars else structs[base]
        if base.startswith("ud_"):
            _refuse(f"{base} is used before it is declared", decl)
        if stars == 0 and base in _SCALARS:
            return _SCALARS[base]
        if stars and base in _POINTEES:
            return C.c_void_p
        _refuse("unknown type", decl)

    def declarator(decl):
        m = _DECL.fullmatch(decl.strip())
        if not m or m["name"] in _KEYWORDS:
            _refuse("unknown declarator", decl)
        t = ctype(decl, m["base"], m["stars"].count("*"))
        return (t * int(m["n"]) if m["n"] else t), m["name"], m

    src, pos = "\n".join(code), 0
    while m := _STMT.match(src, pos):
        pos, stmt = m.end(), m.group(0)
        if m["struct"]:
            fields = []
            for decl in filter(str.strip, m["body"].split(";")):
                first, *more = decl.split(",")
                t, name, d = declarator(first)
                fields.append((name, t))
                for extra in more:                       # `int M, N, K;`: plain names (or arrays) of a pointer-free type
                    e = _MORE.fullmatch(extra.strip())
                    if not e or d["stars"]:
                        _refuse("unknown declarator", decl)
                    t0 = ctype(decl, d["base"], 0)
                    fields.append((e["name"], t0 * int(e["n"]) if e["n"] else t0))
            if m["struct"] in structs:
                _refuse("declared twice", m["struct"])
            structs[m["struct"]] = type(m["struct"], (C.Structure,), {"_fields_": fields})
        elif _HANDLE.fullmatch(m["plain"].strip()):
            handles.add(_HANDLE.fullmatch(m["plain"].strip())["name"])
        else:
            p = _PROTO.fullmatch(m["plain"].strip())
            if not p:
                _refuse("not a prototype the reader knows", stmt)
            if p["name"] in protos:
                _refuse("declared twice", p["name"])
            args = p["args"].strip()
            protos[p["name"]] = (_SCALARS[p["ret"]],
                                 [] if args == "void" else [declarator(a)[:2] for a in args.split(",")])
    if src[pos:].strip():
        _refuse("unterminated or unknown declaration", src[pos:].strip()[:200])
    return Header(protos, structs, consts)


def _read():
    try:
        with open(HEADER_PATH) as f:
            return read_header(f.read())
    except OSError as e:
        raise UDLibraryError(f"the C header of the library cannot be read ({e}); the binding is derived from it") from e


_abi = _read()       # once per process; a few milliseconds


def const(name, consts=None):
    """The integer value of `#define UD_NAME` in the header (consts: another reader result's, for tests)."""
    v = (_abi.consts if consts is None else consts).get(name)
    if not isinstance(v, int):
        raise UDLibraryError(f"include/unidefense_hip.h defines no integer {name}" + ("" if v is None else f": `{v}`"))
    return v


def const_rows(prefix):
    """{lower-cased suffix: value} of the defines that start with prefix, in the header's order (a table's row names)"""
    return {n[len(prefix):].lower(): const(n) for n in _abi.consts if n.startswith(prefix)}


ConvGeom = _abi.structs["ud_conv_geom"]
GemmDesc = _abi.structs["ud_gemm_desc"]
GemmP3Desc = _abi.structs["ud_gemm_p3_desc"]
SplitItem = _abi.structs["ud_split_item"]          # one weight matrix of ud_split_planes_h2t_multi's device table
LayoutItem = _abi.structs["ud_layout_item"]        # one conv weight of ud_weight_layouts_multi's device table
BnRef = _abi.structs["ud_bn_ref"]                  # a deferred BatchNorm, applied by the consuming kernel
LossTail = _abi.structs["ud_loss_tail"]            # the scalar tail of a pass's loss (ud_loss_tail_run)
WgradFold = _abi.structs["ud_wgrad_fold"]          # one item of ud_param_fold_multi: a launch that only finishes a parameter's gradient

EXPORTED = tuple(_abi.protos)

_lib = None


def load():
    """Load (once) and return the ctypes library; raises UDLibraryError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise UDLibraryError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C unidefense_amd/csrc`. unidefense_amd has no fallback path.")
    # The library is linked against /opt/rocm's libamdhip64 while torch ships its own copy.  Loading it BEFORE torch
    # has initialised its HIP runtime leaves this library's kernels registered with a runtime that owns no device
    # (every launch then fails with hipErrorNoDevice) — measured with build() followed by smoke() in one process.
    # So: let torch bring the GPU up first (a no-op on a box without one, where only the symbol table is checked).
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    lib = C.CDLL(LIB_PATH)
    for name, (restype, params) in _abi.protos.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise UDLibraryError(f"{LIB_PATH} does not export {name}; rebuild it")
        fn.argtypes = [t for t, _ in params]
        fn.restype = restype
    _lib = lib
    return lib


def check(status: int, name: str):
    if status != 0:
        raise UDLibraryError(f"{name} failed with status {status}"
                             + (" (invalid argument)" if status == const("UD_EINVAL") else " (-hipError_t)"))


def call(name: str, *args):
    """Call an entry point by the header's convention: a negative result is a failure and raises; anything else (0 of a
    status, the non-negative count of a helper) is returned.  ud_conv_mfma_mode, whose -1 is an answer, is called directly."""
    st = getattr(load(), name)(*args)
    if st < 0:
        check(st, name)
    return st
