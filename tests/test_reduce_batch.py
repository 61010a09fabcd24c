"""CPU: ops.ReduceBatch hands nvit_colsum_reduce_multi no more items than the kernel's argument struct holds
(NVIT_COLSUM_REDUCE_MAX_ITEMS of include/nvit_hip.h): it flushes when that many are collected.  The two launches are
replaced by recorders, so no device and no library is needed."""
import os
import re
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_ITEMS = int(re.search(r"^#define NVIT_COLSUM_REDUCE_MAX_ITEMS[ \t]+(\d+)",
                          open(os.path.join(ROOT, "include", "nvit_hip.h")).read(), flags=re.M).group(1))


def _recorders(monkeypatch):
    from nvit_amd import _lib, ops
    single, multi = [], []

    def reduce_multi(*args):
        assert len(args) == len(_lib.SIGNATURES["nvit_colsum_reduce_multi"])
        n = args[10]
        assert all(len(a) == n for a in args[:10])   # ten host arrays of n entries each
        multi.append(n)
        return 0

    monkeypatch.setattr(ops, "colsum_reduce", lambda part, out, *a, **k: single.append((part, out)))
    monkeypatch.setattr(ops._lib, "load", lambda: types.SimpleNamespace(nvit_colsum_reduce_multi=reduce_multi))
    monkeypatch.setattr(ops, "_s", lambda: None)
    return ops, single, multi


def test_flushes_at_the_kernels_item_limit(monkeypatch):
    ops, single, multi = _recorders(monkeypatch)
    assert MAX_ITEMS >= 2
    rb = ops.ReduceBatch()
    parts = [torch.zeros(3, 4) for _ in range(2 * MAX_ITEMS + 1)]
    outs = [torch.zeros(4) for _ in parts]
    for i in range(MAX_ITEMS - 1):
        rb.add(parts[i], outs[i])
    assert multi == [] and single == [] and len(rb.items) == MAX_ITEMS - 1
    rb.add(parts[MAX_ITEMS - 1], outs[MAX_ITEMS - 1])            # the MAX_ITEMS-th item goes out with the rest
    assert multi == [MAX_ITEMS] and rb.items == []
    for i in range(MAX_ITEMS, 2 * MAX_ITEMS + 1):
        rb.add(parts[i], outs[i])
    assert multi == [MAX_ITEMS, MAX_ITEMS] and len(rb.items) == 1
    rb.flush()                                                     # a single plain item takes the one-reduction entry point
    assert multi == [MAX_ITEMS, MAX_ITEMS] and len(single) == 1 and single[0][0] is parts[-1] and single[0][1] is outs[-1]
    rb.flush()
    assert multi == [MAX_ITEMS, MAX_ITEMS] and len(single) == 1


def test_a_single_item_with_a_second_partial_array_goes_through_the_multi_call(monkeypatch):
    ops, single, multi = _recorders(monkeypatch)
    rb = ops.ReduceBatch()
    rb.add(torch.zeros(3, 4), torch.zeros(4), part_b=torch.zeros(2, 4))
    rb.flush()
    assert multi == [1] and single == []
