"""CPU: the C-ABI shared library builds (hipcc cross-compiles gfx950 without a GPU), loads, and exports every
symbol declared in include/nvit_hip.h with the argument and return types the ctypes table binds.  No compute calls."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_CTYPES_CLASS = {ctypes.c_void_p: "pointer", ctypes.c_char_p: "pointer", ctypes.c_int: "int", ctypes.c_uint: "unsigned",
                 ctypes.c_int64: "int64_t", ctypes.c_uint64: "uint64_t", ctypes.c_float: "float", ctypes.c_double: "double",
                 None: "void"}


def _type_class(decl: str) -> str:
    """The type class of a C parameter declaration (`const float* x`, `int64_t n`, `unsigned`) or of a return type."""
    if "*" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    if len(words) > 1:   # a parameter: the last word is its name
        words = words[:-1]
    cls = " ".join(words)
    assert cls in ("int", "unsigned", "int64_t", "uint64_t", "float", "double", "void"), decl
    return cls


def _declared():
    """name -> (return type class, [argument type classes]) of every entry point the header declares."""
    h = open(os.path.join(ROOT, "include", "nvit_hip.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"(int64_t|int|void|const char\*)\s+(nvit_\w+)\s*\(([^;]*?)\)\s*;", h):
        a = args.strip()
        out[name] = (_type_class(ret), [] if a in ("void", "") else [_type_class(x) for x in a.split(",")])
    return out


def _lib_path():
    from nvit_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return _lib.LIB_PATH


def test_every_declared_symbol_is_exported_and_bound():
    from nvit_amd import _lib
    decl = _declared()
    assert len(decl) >= 40
    lib = ctypes.CDLL(_lib_path())
    for name, (ret, args) in decl.items():
        assert hasattr(lib, name), f"{name} declared in include/nvit_hip.h but not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes binding"
        bound = [_CTYPES_CLASS[t] for t in _lib.SIGNATURES[name]]
        assert len(bound) == len(args), f"{name}: header has {len(args)} args, binding {len(bound)}"
        wrong = [(i, a, b) for i, (a, b) in enumerate(zip(args, bound)) if a != b]
        assert not wrong, f"{name}: (argument index, header type, bound type) {wrong}"
        bound_ret = _CTYPES_CLASS[_lib._RESTYPES.get(name, ctypes.c_int)]
        assert bound_ret == ret, f"{name}: header returns {ret}, binding {bound_ret}"
    for name in _lib.SIGNATURES:
        assert name in decl, f"{name} bound in _lib.py but not declared in the header"
    assert lib.nvit_version() >= 100
    loaded = _lib.load()
    assert loaded.nvit_prof_name(0) == b"gemm_nt"


def test_product_path_never_imports_the_oracle():
    """nvit_amd/ (the product) must not import, call or link anything under oracle/."""
    for dirpath, _, files in os.walk(os.path.join(ROOT, "nvit_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
                assert not re.search(r"(import_module|__import__)\(.*oracle", src), f


def test_model_refuses_to_run_without_a_gpu_tensor():
    import pytest
    import torch
    from nvit_amd.config import named_config
    from nvit_amd.model import ViT
    m = ViT(named_config("micro"))
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 32, 32))
    from nvit_amd.train import normalize_matrices
    with pytest.raises(RuntimeError):
        normalize_matrices(m)


def test_product_sources_carry_no_probe_switches():
    """Timing probes (cut-down kernels whose results are garbage by design) are their own translation units under
    tools/probes/: no NVIT_PROBE switch exists in the product sources, so no -D can turn libnvit_hip.so into one, and
    the library is built from exactly the files the Makefile lists."""
    import glob
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "nvit_amd", "csrc")
    files = glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")) + [os.path.join(root, "include", "nvit_hip.h")]
    assert len(files) > 10
    for f in files:
        hits = [ln for ln in open(f) if re.search(r"#\s*if.*NVIT_PROBE", ln)]
        assert not hits, (f, hits[:3])
        # ... and no other compile-time experiment switch either: the only NVIT_* macros a conditional may test are the
        # product-build guard and include guards (run-time switches go through nvit_set_* / environment variables)
        cond = [ln for ln in open(f) if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b.*\bNVIT_", ln)
                and not re.search(r"NVIT_PRODUCT_BUILD|NVIT_[A-Z_]*_H_?\b", ln)]
        assert not cond, (f, cond[:3])
    mk = open(os.path.join(csrc, "Makefile")).read()
    listed = set(re.search(r"^SRCS\s*=\s*(.*)$", mk, re.M).group(1).split())
    assert listed == {os.path.basename(f) for f in glob.glob(os.path.join(csrc, "*.hip"))}
    # Run-time switches: a selection between a measured winner and a losing variant is not left to the environment (the
    # losing path goes with the option).  What remains read is listed here; every line that touches the environment must
    # name its variable literally.
    def env_reads(paths, pattern):
        names = set()
        for f in paths:
            for ln in open(f):
                if re.search(r"\bgetenv\b|\benviron\b", ln):
                    found = re.findall(pattern, ln)
                    assert found, (f, ln)
                    names.update(found)
        return names
    assert env_reads(files, r'\bgetenv\s*\(\s*"(\w+)"\s*\)') == {"NVIT_XGMI_BLOCKS"}
    py_env = r'\benviron(?:\.get\s*\(|\s*\[)\s*["\'](\w+)["\']'
    assert env_reads(glob.glob(os.path.join(root, "nvit_amd", "*.py")), py_env) == \
        {"NVIT_LIB", "NVIT_PRECISION", "NVIT_GEMM_SCHED", "NVIT_XGMI_TIMEOUT_S"}
    assert env_reads(glob.glob(os.path.join(csrc, "gen", "*.py")), py_env) == {"GEN_PROBE"}


def test_generated_attention_loop_is_reproducible_and_barrier_balanced():
    """The hand-placed dK/dV main loop is a GENERATED inline-asm statement (nvit_amd/csrc/gen/gen_attn_dkv32_asm.py ->
    attn_dkv32_asm.inc, committed).  (1) the committed file is what the generator writes; (2) interpreting its scalar control
    flow for every wave role (computing wave / wave without keys) and tile counts incl. ragged and short last tiles, each
    role executes the same number of s_barrier - a mismatch would hang the workgroup on the GPU - and the computing wave
    issues the expected number of MFMAs."""
    import importlib.util, subprocess, sys
    csrc = os.path.join(ROOT, "nvit_amd", "csrc")
    env = {k: v for k, v in os.environ.items() if k != "GEN_PROBE"}
    out = subprocess.run([sys.executable, os.path.join(csrc, "gen", "gen_attn_dkv32_asm.py")], capture_output=True, text=True,
                         env=env, check=True).stdout
    assert out == open(os.path.join(csrc, "attn_dkv32_asm.inc")).read(), "attn_dkv32_asm.inc is stale: make -C nvit_amd/csrc gen"
    spec = importlib.util.spec_from_file_location("asm_barrier_sim", os.path.join(ROOT, "tools", "probes", "asm_barrier_sim.py"))
    sim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sim)
    ins = sim.load(os.path.join(csrc, "attn_dkv32_asm.inc"))
    for T in (16, 33, 49, 64, 65, 96, 128, 200, 784, 833):
        nt = (T + 63) // 64
        nvl = T - (nt - 1) * 64
        res = {}
        for act in (1, 0):
            for w in range(4):
                res[(act, w)] = sim.run(ins, {6: nt, 9: nvl, 10: act, 11: w * 1024, 8: 0, 7: 1536})
        assert len({r["s_barrier"] for r in res.values()}) == 1, (T, {k: r["s_barrier"] for k, r in res.items()})
        # per full tile 64 MFMAs; the last tile runs 72 (full) or 40 (short) counting the pre-step and the drain
        assert res[(1, 0)]["mfma"] == (nt - 1) * 64 + (40 if nvl <= 32 else 72), (T, res[(1, 0)]["mfma"])
        assert res[(0, 0)]["mfma"] == 0 and res[(1, 0)]["dma"] == 5 * nt
