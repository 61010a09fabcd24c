"""CPU: nvit_amd._lib binds the C ABI from include/nvit_hip.h alone - the prototype grammar and what it refuses, what it
derives from the real header, and _lib.call: the marshalling of tensors, its guards, and the status check.  No launch:
the calls made here are host-only switches or argument refusals that return before any HIP call."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYNTHETIC = """
/* int nvit_in_a_comment(int n); */
#define NVIT_KID_B 1
#define NVIT_KID_A 0   /* int nvit_also_commented(int n); */
#define NVIT_KID_COUNT 2
int nvit_spread(unsigned epoch,
                const int64_t* part,
                void* stream);
const char* nvit_text(uint64_t seed, double x, float y, int64_t n);
void nvit_nothing(void);
int64_t nvit_empty();
"""


@pytest.fixture(scope="module")
def lib():
    from nvit_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    _lib.load()
    return _lib


def test_parser_on_synthetic_header_text():
    from nvit_amd import _lib
    sig, res, params = _lib.parse_prototypes(SYNTHETIC)
    assert list(sig) == ["nvit_spread", "nvit_text", "nvit_nothing", "nvit_empty"]   # nothing from inside a comment
    assert sig["nvit_spread"] == [ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p]
    assert params["nvit_spread"] == ["epoch", "part", "stream"]
    assert sig["nvit_text"] == [ctypes.c_uint64, ctypes.c_double, ctypes.c_float, ctypes.c_int64]
    assert params["nvit_text"] == ["seed", "x", "y", "n"]
    assert sig["nvit_nothing"] == [] and sig["nvit_empty"] == [] and params["nvit_nothing"] == params["nvit_empty"] == []
    assert res == {"nvit_text": ctypes.c_char_p, "nvit_nothing": None, "nvit_empty": ctypes.c_int64}   # int is the default
    assert _lib.kid_names(_lib.parse_constants(SYNTHETIC)) == ["a", "b"]


@pytest.mark.parametrize("text, needles", [
    ("int nvit_x(size_t n);", ("nvit_x", "size_t n")),
    ("int nvit_x(int a, long long n);", ("nvit_x", "long long n")),
    ("int nvit_x(int);", ("nvit_x", "`int`")),
    ("int nvit_x(float*);", ("nvit_x", "float*")),
    ("size_t nvit_x(int n);", ("nvit_x", "size_t")),
    ("float* nvit_x(int n);", ("nvit_x", "float*")),
])
def test_parser_refuses_what_is_outside_the_grammar(text, needles):
    from nvit_amd import _lib
    with pytest.raises(ImportError) as e:
        _lib.parse_prototypes(text, "some/header.h")
    assert "some/header.h" in str(e.value) and all(n in str(e.value) for n in needles), str(e.value)


def test_kernel_family_values_must_count_up_without_a_gap():
    from nvit_amd import _lib
    for text in ("#define NVIT_KID_A 0\n#define NVIT_KID_B 2\n#define NVIT_KID_COUNT 2\n",     # a gap
                 "#define NVIT_KID_A 0\n#define NVIT_KID_B 0\n#define NVIT_KID_COUNT 2\n",     # a value twice
                 "#define NVIT_KID_A 0\n#define NVIT_KID_B 1\n#define NVIT_KID_COUNT 3\n",     # fewer than COUNT
                 "#define NVIT_KID_A 0\n#define NVIT_KID_B 1\n"):                              # no COUNT
        with pytest.raises(ImportError) as e:
            _lib.kid_names(_lib.parse_constants(text), "some/header.h")
        assert "some/header.h" in str(e.value) and "NVIT_KID_" in str(e.value)


def test_real_header():
    from nvit_amd import _lib
    from test_row_gate_refusals import ARGS
    assert len(ARGS) == 6
    for name, names in ARGS.items():
        assert _lib.PARAMS[name] == names.split(), name
    assert _lib.KID_NAMES[10] == "gemm_swiglu" and len(_lib.KID_NAMES) == _lib.HEADER["KID_COUNT"]
    assert (_lib.F32, _lib.BF16, _lib.BF16_F32IN) == (0, 1, 3)
    assert len(_lib.SIGNATURES) >= 100 and set(_lib.PARAMS) == set(_lib.SIGNATURES) >= set(_lib._RESTYPES)
    for name, sig in _lib.SIGNATURES.items():
        assert len(sig) == len(_lib.PARAMS[name]), name
    assert _lib.SIGNATURES["nvit_lerp_fwd"][:3] == [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    assert _lib.SIGNATURES["nvit_lerp_fwd"][5] is ctypes.c_float and _lib.PARAMS["nvit_lerp_fwd"][5] == "c_a"


def test_call_returns_none_and_raises_with_the_entry_point_and_its_message(lib):
    assert lib.call("nvit_set_gemm_impl", -1, -1) is None
    with pytest.raises(RuntimeError) as e:
        lib.call("nvit_set_gemm_impl", 5, 5)
    assert "nvit_set_gemm_impl" in str(e.value) and "nt in -1..2" in str(e.value)
    assert lib.call("nvit_set_gemm_impl", -1, -1) is None


M, C, T = 12, 64, 3   # the valid shape of test_row_gate_refusals


def _lerp_fwd_args(**over):
    """a gated nvit_lerp_fwd call on host tensors: only ever handed to a call that is refused before it launches"""
    t = lambda *shape: torch.zeros(*shape)
    vals = dict(dt=1, h=t(M, C), y=t(M, C), y_dt=1, alpha=torch.nn.Parameter(t(C)), c_a=1.0, skip_x=None, skip=None,
                gate=t(M // T), rows_per_sample=0, out=t(M, C), out_lo=t(M, C), M=M, C=C, stream=None)
    vals.update(over)
    return list(vals.values())


def test_call_marshals_tensors_parameters_and_none(lib):
    assert list(lib.PARAMS["nvit_lerp_fwd"]) == "dt h y y_dt alpha c_a skip_x skip gate rows_per_sample out out_lo M C stream".split()
    with pytest.raises(RuntimeError) as e:
        lib.call("nvit_lerp_fwd", *_lerp_fwd_args())
    assert "nvit_lerp_fwd" in str(e.value) and "rows_per_sample=0" in str(e.value)
    with pytest.raises(RuntimeError) as e:       # the ints arrive where they belong: M = 12 is no multiple of 5
        lib.call("nvit_lerp_fwd", *_lerp_fwd_args(rows_per_sample=5))
    assert "rows_per_sample=5" in str(e.value)


def test_call_guards(lib, monkeypatch):
    made = []

    class Recorder:
        def __getattr__(self, name):
            return lambda *a: made.append(name) or 0

    monkeypatch.setattr(lib, "load", lambda: Recorder())
    with pytest.raises(TypeError) as e:      # a tensor's address in an int parameter would be truncated without a word
        lib.call("nvit_lerp_fwd", *_lerp_fwd_args(M=torch.zeros(1)))
    assert "nvit_lerp_fwd" in str(e.value) and "`M`" in str(e.value)
    with pytest.raises(TypeError) as e:
        lib.call("nvit_lerp_fwd", *_lerp_fwd_args()[:-1])
    assert "nvit_lerp_fwd" in str(e.value) and "rows_per_sample" in str(e.value) and "stream" in str(e.value)
    with pytest.raises(TypeError):
        lib.call("nvit_lerp_fwd", *_lerp_fwd_args(), None)
    # entry points that return a value, not a status: an int-valued query, and every other return type
    for name, args in (("nvit_gemm_nt_fusable", (1, 256, 256, 256)), ("nvit_crop_ws_bytes", (1, 8, 8, 3, 4, 0)),
                       ("nvit_version", ()), ("nvit_lerp_bwd_blocks", (1, 1, 64, 0, 1, 0, 0)), ("nvit_patch_embed_kp", (48,)),
                       ("nvit_last_error", ()), ("nvit_prof_enable", (0,)), ("nvit_no_such_entry_point", ())):
        with pytest.raises(TypeError) as e:
            lib.call(name, *args)
        assert name in str(e.value)
    assert made == []
    lib.call("nvit_set_gemm_impl", -1, -1)
    assert made == ["nvit_set_gemm_impl"]     # the recorder does see a call that passes the guards


def test_every_value_returning_entry_point_is_refused_by_call(lib):
    """The issue's list: these return values, so a non-zero result is no error and `call` must not read it as one."""
    values = {"nvit_version", "nvit_last_error", "nvit_prof_name", "nvit_prof_enable", "nvit_prof_select",
              "nvit_gemm_nt_fusable", "nvit_lerp_bwd_blocks", "nvit_patch_embed_kp", "nvit_crop_ws_bytes",
              "nvit_center_crop_ws_bytes", "nvit_xgmi_chunk", "nvit_xgmi_flag_bytes"}
    assert values <= set(lib.SIGNATURES)
    assert set(lib.SIGNATURES) - set(lib._POINTERS) == values
