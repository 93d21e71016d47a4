"""The C-ABI library loads on a CPU-only host and exports every declared symbol."""

import ctypes
import os
import re

from specdec_hip import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    names = set()
    inc = os.path.join(ROOT, "include")
    for fn in os.listdir(inc):
        if fn.endswith(".h"):
            text = open(os.path.join(inc, fn)).read()
            text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
            names |= set(re.findall(r"\b(sd_[a-z0-9_]+)\s*\(", text))
    return names


def test_library_exports_every_header_symbol():
    lib = _abi.load()
    declared = _declared_symbols()
    assert declared, "no sd_* declarations found in include/*.h"
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/ but not exported"
    # and the binding table covers the header exactly
    assert declared == set(_abi.SIGNATURES), declared ^ set(_abi.SIGNATURES)


def test_abi_version_and_error_string():
    lib = _abi.load()
    assert lib.sd_abi_version() == _abi.SD_ABI_VERSION
    assert isinstance(_abi.last_error(), str)


def test_argument_validation_without_gpu():
    """Validation errors are reported through the return code + sd_last_error, before
    any device work (so this is safe on a host without a GPU)."""
    lib = _abi.load()
    rc = lib.sd_kv_append(None, None, None, None, None, 0, 3, 1, 1, 8, 1, 4, None)
    assert rc != 0 and "elem_size" in _abi.last_error()
    rc = lib.sd_verify_prefix(None, 99, None, _abi.SD_I64, ctypes.c_void_p(8), None, None,
                              1, 1, 10, 10, 10, None, 0, None)
    assert rc != 0 and "NULL" in _abi.last_error() or "dtype" in _abi.last_error()
    assert lib.sd_verify_prefix_workspace(2, 4, 1000) >= 2 * 4 * 8


_C_KINDS = {"int": "i32", "int32_t": "i32", "int64_t": "i64", "long": "i64", "long long": "i64", "unsigned": "u32", "unsigned int": "u32",
            "uint32_t": "u32", "uint64_t": "u64", "size_t": "u64", "float": "f32", "double": "f64"}


def _c_kind(decl, named):
    """Kind of one C parameter (`named`: its last word is the parameter's name) or return type."""
    if "*" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    return _C_KINDS[" ".join(words[:-1] if named else words)]


def _header_prototypes():
    text = open(os.path.join(ROOT, "include", "specdec_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"^\s*#[^\n]*", "", text, flags=re.M)
    protos = {}
    for stmt in re.split(r"[;{}]", text):
        m = re.fullmatch(r"\s*([A-Za-z_][\w\s\*]*?)\s*\b(sd_[a-z0-9_]+)\s*\(([^()]*)\)\s*", stmt)
        if not m:
            continue
        ret, name, params = m.groups()
        assert name not in protos, f"{name} is declared twice"
        params = [p.strip() for p in params.split(",")]
        args = [] if params in ([""], ["void"]) else [_c_kind(p, True) for p in params]
        protos[name] = (_c_kind(ret, False), args)
    return protos


def _ctypes_kind(t):
    if issubclass(t, (ctypes._Pointer, ctypes.c_void_p, ctypes.c_char_p)):
        return "pointer"
    if t in (ctypes.c_float, ctypes.c_double):
        return f"f{8 * ctypes.sizeof(t)}"
    return ("i" if t(-1).value < 0 else "u") + str(8 * ctypes.sizeof(t))


def test_binding_matches_header_prototypes():
    """Every entry of _abi.SIGNATURES has the header's return and argument kinds (pointer / i32 / i64 / u32 / u64 / f32 / f64):
    a wrong width in an argtype would pass garbage without an error."""
    protos = _header_prototypes()
    assert set(protos) == set(_abi.SIGNATURES), set(protos) ^ set(_abi.SIGNATURES)
    for name, (restype, argtypes) in sorted(_abi.SIGNATURES.items()):
        bound = (_ctypes_kind(restype), [_ctypes_kind(t) for t in argtypes])
        assert bound == protos[name], f"{name}: the binding has {bound}, the header {protos[name]}"
