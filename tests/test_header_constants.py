"""CPU: include/nvit_hip.h is the one place where a number shared by the host and the kernels is written.  The header is
parsed here on its own (not through nvit_amd._lib) and compared with what the Python modules hold."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _macros():
    out = {}
    for ln in open(os.path.join(ROOT, "include", "nvit_hip.h")):
        parts = ln.split()
        if len(parts) >= 3 and parts[0] == "#define" and parts[1].startswith("NVIT_"):
            try:
                out[parts[1][len("NVIT_"):]] = int(parts[2], 10)
            except ValueError:
                pass
    return out


def test_every_integer_macro_is_exposed_with_its_value():
    from nvit_amd import _lib
    macros = _macros()
    assert len(macros) >= 50 and macros["EINVAL"] == 1001 and macros["KID_COUNT"] == 15
    assert _lib.HEADER == macros
    for name, value in macros.items():
        assert _lib.const(name) == value


def test_a_missing_name_fails_with_the_file_and_the_name():
    from nvit_amd import _lib
    with pytest.raises(ImportError) as e:
        _lib.const("NO_SUCH_CONSTANT")
    assert "nvit_hip.h" in str(e.value) and "NVIT_NO_SUCH_CONSTANT" in str(e.value)


def test_a_missing_header_fails_with_the_file(monkeypatch):
    from nvit_amd import _lib
    monkeypatch.setattr(_lib, "HEADER_PATH", os.path.join(ROOT, "include", "not_there.h"))
    with pytest.raises(ImportError) as e:
        _lib._header_constants()
    assert "not_there.h" in str(e.value)


def test_python_names_equal_their_macros():
    from nvit_amd import _lib, augment, mix, ops, optim
    m = _macros()
    kept = {
        (_lib, "RENORM_ROWS_PER_ITEM"): "RENORM_ROWS_PER_ITEM", (_lib, "RENORM_COLS_PER_ITEM"): "RENORM_COLS_PER_ITEM",
        (_lib, "RENORM_TALL_ROWS"): "RENORM_TALL_ROWS", (_lib, "RENORM_TALL_COLS_PER_ITEM"): "RENORM_TALL_COLS_PER_ITEM",
        (_lib, "RENORM_MAX_ROWS_DIM0"): "RENORM_MAX_ROWS_DIM0", (_lib, "MAX_EMBD"): "MAX_EMBD",
        (_lib, "ATTN_HEADS_MAX_H"): "ATTN_HEADS_MAX_H",
        (ops, "PAD_HEAD_DIM"): "PAD_HEAD_DIM", (ops, "MAX_PART_BLOCKS"): "MAX_PART_BLOCKS", (ops, "ROW_WAVES"): "ROW_WAVES",
        (ops, "REDUCE_MAX_ITEMS"): "COLSUM_REDUCE_MAX_ITEMS", (ops, "ATTN_BWD_PART_ROWS"): "ATTN_BWD_PART_ROWS",
        (ops, "SWIGLU_BWD_TILE_ROWS"): "SWIGLU_BWD_TILE_ROWS", (ops, "SWIGLU_BWD_PART_ROWS"): "SWIGLU_BWD_PART_ROWS",
        (ops, "PATCH_K_STEP"): "PATCH_EMBED_K_STEP", (ops, "PATCH_TILE_ROWS"): "PATCH_EMBED_TILE_ROWS",
        (ops, "SHADOW_TILE"): "SHADOW_TILE",
        (augment, "ROW"): "AUG_ROW", (augment, "MAX_SIDE"): "AUG_MAX_SIDE", (augment, "N_MAGNITUDES"): "AUG_NMAG",
        (mix, "ROW"): "MIX_ROW", (mix, "KNOTS"): "MIX_KNOTS",
        (optim, "_TABLE_COLS"): "OPT_TABLE_COLS", (optim, "_CHUNK"): "OPT_CHUNK", (optim, "_ROWS_PER_ITEM"): "OPT_ROWS_PER_ITEM",
        (optim, "_SLAB_COLS"): "OPT_SLAB_COLS", (optim, "_SLAB_ROWS"): "OPT_SLAB_ROWS", (optim, "_TALL_COLS"): "OPT_TALL_COLS",
        (optim, "_TALL_ROWS"): "OPT_TALL_ROWS", (optim, "_ROW_COLS"): "OPT_ROW_COLS", (optim, "_WIDE_COLS"): "OPT_WIDE_COLS",
        (optim, "_WIDE_LDS_ROWS"): "OPT_WIDE_LDS_ROWS",
    }
    for (mod, name), macro in kept.items():
        v = getattr(mod, name)
        assert type(v) is int and v == m[macro], (mod.__name__, name, v, macro, m[macro])
    assert len(augment.OPS) == m["AUG_NOPS"]
    assert len(_lib.KID_NAMES) == m["KID_COUNT"]
    assert (_lib.F32, _lib.BF16, _lib.BF16_F32IN) == (m["F32"], m["BF16"], m["BF16_F32IN"])
    # host choices that a kernel limits stay inside the limit
    assert ops.PART_BLOCKS <= m["MAX_PART_BLOCKS"] and optim._NPART <= m["OPT_MAX_PART"]
    assert ops.ATTN_HEADS_BWD_BLOCKS <= m["ATTN_HEADS_BWD_MAX_BLOCKS"]
    assert ops.patch_kp(1) == m["PATCH_EMBED_K_STEP"] and ops.patch_kp(m["PATCH_EMBED_K_STEP"] + 1) == 2 * m["PATCH_EMBED_K_STEP"]
