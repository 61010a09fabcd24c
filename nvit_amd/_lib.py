"""ctypes binding of libnvit_hip.so, derived from the C ABI's one declaration: include/nvit_hip.h.

The header's `#define NVIT_<NAME> <integer>` lines and its prototypes are parsed at import (DESIGN.md §3 states the
grammar): no entry point's argument list is restated here.  `call` is the one way to make a status-returning call.

The product path has NO CPU or PyTorch fallback: if the library is missing or a call
fails, a RuntimeError is raised.
"""
from __future__ import annotations

import ctypes as C
import os
import re

from torch import Tensor

_HERE = os.path.dirname(os.path.abspath(__file__))
# (NVIT_LIB: experiments with an alternative build of the same sources, e.g. tools/ab_lib.sh; never set in product use)
LIB_PATH = os.environ.get("NVIT_LIB") or os.path.join(_HERE, "libnvit_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "nvit_hip.h")


_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float,
            "double": C.c_double}
_RETURNS = {**_SCALARS, "void": None, "char*": C.c_char_p}
_PROTOTYPE = re.compile(r"([\w*][\w* \t]*?)\s*\b(nvit_\w+)\s*\(([^;()]*)\)\s*;")


def parse_constants(text: str) -> dict:
    """name without the NVIT_ prefix -> value of every `#define NVIT_<NAME> <integer>` of the header text."""
    return {name: int(value) for name, value in re.findall(r"#define NVIT_(\w+)\s+(-?\d+)", text)}


def _words(decl: str) -> str:
    return " ".join(w for w in decl.replace("*", "* ").split() if w != "const").replace(" *", "*")


def parse_prototypes(text: str, where: str = "the header"):
    """-> (SIGNATURES, _RESTYPES, PARAMS) of every `<type> nvit_<name>(<type> <name>, ...);` outside /* */ comments.
    A `*` anywhere in a parameter makes it a c_void_p; the scalar types are _SCALARS; `const` is ignored and the last
    word is the parameter's name.  Anything else is refused: a declaration must never bind as a guess."""
    signatures, restypes, params = {}, {}, {}
    for ret, name, arglist in _PROTOTYPE.findall(re.sub(r"/\*.*?\*/", "", text, flags=re.S)):
        def refuse(decl, why):
            return ImportError(f"nvit_amd: {where}: {name}: cannot bind `{decl}`: {why} (the binding grammar takes "
                               f"pointers, {', '.join(_SCALARS)}, and returns of those, void or const char*)")
        if _words(ret) not in _RETURNS:
            raise refuse(" ".join(ret.split()), "unknown return type")
        if _RETURNS[_words(ret)] is not C.c_int:
            restypes[name] = _RETURNS[_words(ret)]
        signatures[name], params[name] = [], []
        for decl in ([] if arglist.strip() in ("", "void") else arglist.split(",")):
            decl = " ".join(decl.split())
            m = re.fullmatch(r"(.*?)(\w+)", decl)
            kind = _words(m.group(1)) if m else ""
            if not kind:
                raise refuse(decl, "a parameter needs a type and a name")
            if "*" not in kind and kind not in _SCALARS:
                raise refuse(decl, f"unknown type `{kind}`")
            signatures[name].append(C.c_void_p if "*" in kind else _SCALARS[kind])
            params[name].append(m.group(2))
    return signatures, restypes, params


def kid_names(constants: dict, where: str = "the header") -> list:
    """The kernel families of nvit_prof_*: the NVIT_KID_* macros but COUNT, lower-cased, in the order of their values."""
    kids = sorted((v, k[4:].lower()) for k, v in constants.items() if k.startswith("KID_") and k != "KID_COUNT")
    if [v for v, _ in kids] != list(range(constants.get("KID_COUNT", -1))):
        raise ImportError(f"nvit_amd: {where}: the NVIT_KID_* values must be 0..NVIT_KID_COUNT-1 without gaps, got {kids}")
    return [k for _, k in kids]


def _header_text() -> str:
    """The C header's text: importing needs no built library."""
    try:
        with open(HEADER_PATH) as f:
            return f.read()
    except OSError as e:
        raise ImportError(f"nvit_amd: cannot read the C header that declares the kernels' ABI and layout constants: {e}") from None


def _header_constants() -> dict:
    return parse_constants(_header_text())


_TEXT = _header_text()
HEADER = parse_constants(_TEXT)   # name without the NVIT_ prefix -> value
# name -> argtypes; name -> restype where it is not int; name -> parameter names
SIGNATURES, _RESTYPES, PARAMS = parse_prototypes(_TEXT, HEADER_PATH)
del _TEXT


def const(name: str) -> int:
    """NVIT_<name> of include/nvit_hip.h, where every number that host and kernels share is written; for use at import."""
    if name not in HEADER:
        raise ImportError(f"nvit_amd: {HEADER_PATH} has no integer `#define NVIT_{name}`")
    return HEADER[name]


F32, BF16, BF16_F32IN = const("F32"), const("BF16"), const("BF16_F32IN")
KID_NAMES = kid_names(HEADER, HEADER_PATH)
RENORM_ROWS_PER_ITEM = const("RENORM_ROWS_PER_ITEM")
RENORM_COLS_PER_ITEM = const("RENORM_COLS_PER_ITEM")
RENORM_TALL_ROWS = const("RENORM_TALL_ROWS")   # column-normalised matrices with more rows take the narrow panel
RENORM_TALL_COLS_PER_ITEM = const("RENORM_TALL_COLS_PER_ITEM")
RENORM_MAX_ROWS_DIM0 = const("RENORM_MAX_ROWS_DIM0")
MAX_EMBD = const("MAX_EMBD")   # widest row the row kernels hold (lerp, norm_skip, rmsnorm, res_*, qknorm, pool_ln, ...)
ATTN_HEADS_MAX_H = const("ATTN_HEADS_MAX_H")

_lib = None


def bind(cdll: C.CDLL, partial: bool = False) -> C.CDLL:
    """Give every declared entry point of `cdll` its argtypes and restype (partial: skip those an older build lacks)."""
    for name, args in SIGNATURES.items():
        if partial and not hasattr(cdll, name):
            continue
        fn = getattr(cdll, name)  # AttributeError if the symbol is not exported
        fn.argtypes = args
        fn.restype = _RESTYPES.get(name, C.c_int)
    return cdll


def load() -> C.CDLL:
    """Load the HIP library; raise loudly when it is absent (no fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"nvit_amd: {LIB_PATH} not found. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the nViT hot path.")
    _lib = bind(C.CDLL(LIB_PATH))
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().nvit_last_error()
        raise RuntimeError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")


# entry points that return an int VALUE, not a status: like every non-int return they are called as load().nvit_x(...)
_INT_QUERIES = frozenset({"nvit_version", "nvit_gemm_nt_fusable", "nvit_lerp_bwd_blocks", "nvit_patch_embed_kp"})
# status-returning entry point -> per parameter, whether the header declares a pointer
_POINTERS = {name: tuple(t is C.c_void_p for t in args) for name, args in SIGNATURES.items()
             if name not in _RESTYPES and name not in _INT_QUERIES}


def call(name: str, *args) -> None:
    """Make the status-returning call `name(*args)`: tensors go as their data_ptr() and only into pointer parameters,
    everything else (None, numbers, ctypes arrays, byref) goes as it is; a non-zero status raises with nvit_last_error()."""
    pointers = _POINTERS.get(name)
    if pointers is None:
        raise TypeError(f"{name} is not a status-returning entry point of {HEADER_PATH}: call it as load().{name}(...)")
    if len(args) != len(pointers):
        raise TypeError(f"{name} takes {len(pointers)} arguments ({', '.join(PARAMS[name])}), got {len(args)}")
    argv = list(args)
    for i, a in enumerate(argv):
        if isinstance(a, Tensor):
            if not pointers[i]:
                raise TypeError(f"{name}: parameter `{PARAMS[name][i]}` is not a pointer, got a tensor")
            argv[i] = a.data_ptr()
    check(getattr(load(), name)(*argv), name)
