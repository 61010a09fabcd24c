"""CPU: the host-built work tables count their items as the kernels walk them, at the edges of the item geometry.  The
expected counts are computed here from the header's values (parsed here, not taken from the modules under test)."""
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = {n: int(v) for n, v in re.findall(r"^#define NVIT_(\w+)[ \t]+(-?\d+)\b", open(os.path.join(ROOT, "include", "nvit_hip.h")).read(),
                                      flags=re.M)}


def _renorm(mats):
    from nvit_amd import ops
    table, total = ops.renorm_table([(torch.zeros(r, c), dim) for r, c, dim in mats], "cpu")
    assert table.shape == (len(mats), 5) and table.dtype == torch.int64
    assert [tuple(row[1:4]) for row in table.tolist()] == [tuple(m) for m in mats]
    firsts = table[:, 4].tolist()
    return [b - a for a, b in zip(firsts, firsts[1:] + [total])], firsts[0]


def test_renorm_table_rows_per_item_edge():
    rpi = H["RENORM_ROWS_PER_ITEM"]
    items, first = _renorm([(rpi, 8, 1), (rpi + 1, 8, 1), (3 * rpi - 1, 4, 1), (1, 4, 1)])
    assert first == 0 and items == [1, 2, 3, 1]


def test_renorm_table_panel_width_follows_the_row_count():
    wide, tall, tall_rows = H["RENORM_COLS_PER_ITEM"], H["RENORM_TALL_COLS_PER_ITEM"], H["RENORM_TALL_ROWS"]
    assert tall < wide
    cols = 2 * wide + 1   # one past a whole panel of either width
    assert cols % tall == 1
    items, _ = _renorm([(tall_rows, cols, 0), (tall_rows + 1, cols, 0), (tall_rows, 2 * wide, 0), (tall_rows + 1, 2 * wide, 0),
                        (H["RENORM_MAX_ROWS_DIM0"], 1, 0)])
    assert items == [3, 2 * wide // tall + 1, 2, 2 * wide // tall, 1]
    assert items[0] == math.ceil(cols / wide) and items[1] == math.ceil(cols / tall)


def test_renorm_table_refuses_a_matrix_taller_than_the_panel():
    from nvit_amd import ops
    with pytest.raises(RuntimeError, match=str(H["RENORM_MAX_ROWS_DIM0"])):
        ops.renorm_table([(torch.zeros(H["RENORM_MAX_ROWS_DIM0"] + 1, 4), 0)], "cpu")
    ops.renorm_table([(torch.zeros(H["RENORM_MAX_ROWS_DIM0"] + 1, 4), 1)], "cpu")   # rows are not limited for dim 1


def test_optimizer_plain_chunks():
    from nvit_amd.optim import table_items
    chunk = H["OPT_CHUNK"]
    assert table_items(-1, 1, chunk) == (1, 1, 0)
    assert table_items(-1, 1, chunk + 1) == (2, 2, 0)
    assert table_items(-1, 1, 1) == (1, 1, 0)


def test_optimizer_row_normalised_items():
    from nvit_amd.optim import table_items
    rpi, chunk = H["OPT_ROWS_PER_ITEM"], H["OPT_CHUNK"]
    assert table_items(1, rpi, 64) == (1, math.ceil(rpi * 64 / chunk), 0)
    assert table_items(1, rpi + 1, 64) == (2, math.ceil((rpi + 1) * 64 / chunk), 0)
    # rows of up to OPT_ROW_COLS columns stay in registers; wider ones are parked in LDS sized as a slab of
    # NVIT_OPT_WIDE_LDS_ROWS rows
    assert table_items(1, 3, H["OPT_ROW_COLS"])[2] == 0
    c = H["OPT_ROW_COLS"] + 4
    assert table_items(1, 3, c) == (1, math.ceil(3 * c / chunk), H["OPT_WIDE_LDS_ROWS"])
    assert table_items(1, 3, H["OPT_WIDE_COLS"])[2] == H["OPT_WIDE_LDS_ROWS"]
    with pytest.raises(RuntimeError, match=str(H["OPT_WIDE_COLS"])):
        table_items(1, 3, H["OPT_WIDE_COLS"] + 4)
    with pytest.raises(RuntimeError):
        table_items(1, 3, 66)   # cols % 4


def test_optimizer_column_normalised_items():
    from nvit_amd.optim import table_items
    slab, tall, slab_rows, chunk = H["OPT_SLAB_COLS"], H["OPT_TALL_COLS"], H["OPT_SLAB_ROWS"], H["OPT_CHUNK"]
    assert tall < slab
    cols = 3 * slab + 1   # one past a whole slab of either width
    assert cols % tall == 1
    assert table_items(0, slab_rows, cols) == (4, math.ceil(slab_rows * cols / chunk), slab_rows)
    assert table_items(0, slab_rows + 1, cols) == (3 * slab // tall + 1, math.ceil((slab_rows + 1) * cols / chunk), slab_rows + 1)
    assert table_items(0, slab_rows, 3 * slab)[0] == 3 and table_items(0, slab_rows + 1, 3 * slab)[0] == 3 * slab // tall
    assert table_items(0, H["OPT_TALL_ROWS"], 1) == (1, 1, H["OPT_TALL_ROWS"])
    with pytest.raises(RuntimeError, match=str(H["OPT_TALL_ROWS"])):
        table_items(0, H["OPT_TALL_ROWS"] + 1, 4)
