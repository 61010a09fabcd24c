"""CPU: the interface of the bias-taking fused GEMM epilogues - the three C entry points take an optional bias and
are declared, exported and bound (test_cabi_symbols.py checks that header and binding agree on every symbol; this one
names them), the ops wrappers take `bias`, and the Base-with-bias configuration exists.  No compute calls."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED = ("nvit_gemm_nt_swiglu", "nvit_gemm_nt_swiglu_act", "nvit_gemm_nt_qknorm")


def test_bias_entry_points_are_declared_exported_and_bound():
    from nvit_amd import _lib
    h = open(os.path.join(ROOT, "include", "nvit_hip.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    lib = _lib.load()
    for name in FUSED:
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, h)
        assert m, f"{name} is not declared in include/nvit_hip.h"
        args = [a.strip() for a in m.group(1).split(",")]
        # `const float* bias` (NULL: none) before the stream
        assert re.fullmatch(r"const\s+float\s*\*\s*bias", args[-2]), (name, args[-2:])
        assert re.fullmatch(r"void\s*\*\s*stream", args[-1]), (name, args[-1])
        assert hasattr(lib, name), f"{name} is not exported"
        sig = _lib.SIGNATURES[name]
        assert len(sig) == len(args) and sig[-2] is ctypes.c_void_p and sig[-1] is ctypes.c_void_p, name
    # one name per epilogue: no second entry point for the biased form, in the header, the binding or the library
    twin = re.compile(r"nvit_gemm_nt_\w+_bias\b")
    assert not twin.search(h)
    assert not [n for n in _lib.SIGNATURES if twin.fullmatch(n)]
    binary = open(_lib.LIB_PATH, "rb").read()           # the dynamic string table holds every exported name
    assert b"\0nvit_gemm_nt_swiglu\0" in binary and not re.search(rb"nvit_gemm_nt_\w+_bias\b", binary)


def test_ops_wrappers_take_a_bias():
    from nvit_amd import ops
    for fn in (ops.gemm_nt_swiglu, ops.gemm_nt_swiglu_act, ops.gemm_nt_qknorm):
        p = inspect.signature(fn).parameters
        assert "bias" in p and p["bias"].default is None, fn.__name__
        assert list(p)[-1] == "bias", fn.__name__


def test_base_b_is_base_with_bias():
    from dataclasses import asdict
    from nvit_amd.config import named_config
    b, base = named_config("base_b"), named_config("base")
    assert b.bias is True and base.bias is False
    assert {k: v for k, v in asdict(b).items() if k != "bias"} == {k: v for k, v in asdict(base).items() if k != "bias"}
