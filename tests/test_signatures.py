"""CPU: every row of _atgpu.SIGNATURES against the prototype of the same name
in include/atgpu.h: parameter count, the kind of every parameter (pointer,
u32, u64, i32, i64, f32, f64, struct by value) and the kind of the result.
The enums atg_pcm_format and atg_status count as i32.  No kernel is launched."""
import ctypes
import re

from audiotools import _atgpu
from test_abi import HEADER, declared_functions

SCALARS = {"uint32_t": "u32", "uint64_t": "u64", "int32_t": "i32", "int64_t": "i64",
           "int": "i32", "float": "f32", "double": "f64", "void": "void",
           "atg_pcm_format": "i32", "atg_status": "i32"}
CTYPES = {ctypes.c_uint32: "u32", ctypes.c_uint64: "u64", ctypes.c_int32: "i32",
          ctypes.c_int64: "i64", ctypes.c_float: "f32", ctypes.c_double: "f64", None: "void",
          ctypes.c_void_p: "pointer", ctypes.c_char_p: "pointer"}


def c_kind(decl, is_parameter):
    """kind of `const uint32_t *sizes`, `atg_pcm_layout layout`, `const char *` ..."""
    if "*" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    if is_parameter and len(words) > 1:
        words = words[:-1]   # the parameter's name
    assert len(words) == 1, decl
    return SCALARS.get(words[0], "struct")


def ctypes_kind(t):
    if t in CTYPES:
        return CTYPES[t]
    if isinstance(t, type) and issubclass(t, ctypes._Pointer):
        return "pointer"
    if isinstance(t, type) and issubclass(t, ctypes.Structure):
        return "struct"
    raise AssertionError("no kind for %r" % (t,))


def prototypes():
    """{name: (result kind, [parameter kinds])} of include/atgpu.h"""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    out = {}
    for result, name, args in re.findall(
            r"([A-Za-z_][\w\s\*]*?)\b(atg_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        args = " ".join(args.split())
        params = [] if args == "void" else [c_kind(a, True) for a in args.split(",")]
        out[name] = (c_kind(result, False), params)
    return out


def test_every_prototype_is_parsed():
    assert sorted(prototypes()) == declared_functions()
    assert len(prototypes()) == 158


def test_table_agrees_with_header():
    protos = prototypes()
    assert sorted(_atgpu.SIGNATURES) == sorted(protos)
    wrong = []
    for name, (result, params) in sorted(protos.items()):
        restype, argtypes = _atgpu.SIGNATURES[name]
        got = (ctypes_kind(restype), [ctypes_kind(t) for t in argtypes])
        if got != (result, params):
            wrong.append((name, (result, params), got))
    assert not wrong, wrong


def test_no_function_keeps_the_default_signature():
    """after load_library() only an `int f(void)` may look as ctypes made it"""
    lib = _atgpu.load_library()
    for name, (result, params) in prototypes().items():
        fn = getattr(lib, name)
        if (result, params) != ("i32", []):
            assert fn.argtypes is not None, name
            assert len(fn.argtypes) == len(params), name
            assert ctypes_kind(fn.restype) == result, name
