"""The oracles of optim_check.py have teeth (CPU only, no GPU): the fp32 restatements of the fused optimizer step (the
plain torch sequence at float32, and `walk`, the two launches item by item in the kernels' order) stay inside the fp64
bounds at every case of test_gpu_optim_bounds.py, the bounds' own values equal the fp64 reference, the reported norm of
exact-sum data is bit-exact, every named mutant falls outside in the case that KILLS names for it, and the tables are what
the kernels walk: every element in exactly one item and one chunk, the hand-offs between consecutive items present."""
import pytest
import torch

import optim_check as oc
import rowops_check as rc

from nvit_amd import ops, optim

F32 = torch.float32


# ------------------------------------------------------------------------------------------------ layouts
def test_constants_are_the_hosts():
    assert oc.NPART == optim._NPART
    assert oc.OPT_GRID == 2048 and oc.R_GRID == 2048
    for t in (oc.EDGES, oc.SWEEP):
        for e in t.entries:
            items, chunks, _ = optim.table_items(e.kind, e.rows, e.cols)
            assert (items, chunks) == (e.items, e.chunks), e.shape
    for mats in (oc.RENORM_SWEEP, oc.RENORM_EDGES):
        ws = [torch.empty(shape) for shape, _ in mats]
        _, items = ops.renorm_table([(w, d) for w, (_, d) in zip(ws, mats)], torch.device("cpu"))
        assert items == sum(oc.renorm_items(r, c, d) for (r, c), d in mats)


@pytest.mark.parametrize("name", ["EDGES", "SWEEP"])
def test_items_and_chunks_cover_every_element_once(name):
    t = getattr(oc, name)
    items, chunks = oc.coverage(t)
    mask = t.mask().numpy()
    assert (items[mask] == 1).all() and (items[~mask] == 0).all()
    assert (chunks[mask] == 1).all() and (chunks[~mask] == 0).all()
    assert mask.sum() == t.n_elems
    assert all(e.off % 4 == 0 for e in t.entries)


def test_edges_holds_every_edge_of_the_issue():
    shapes = {k: {e.shape for e in oc.EDGES.entries if e.kind == k} for k in (-1, 0, 1)}
    assert shapes[1] == {(1, 4), (16, 4), (17, 252), (2, 256), (17, 260), (33, 1536), (5, 1540), (18, 2048)}
    assert shapes[0] == {(1, 1), (1, 33), (7, 32), (127, 31), (129, 35), (1152, 37), (1153, 16), (1153, 17), (2048, 33)}
    assert shapes[-1] == {(1,), (3,), (4,), (8192,), (8193,), (8195,), (16396,), (2, 3, 5, 7)}
    assert oc.EDGES.grid == oc.EDGES.items            # one sweep: no workgroup takes a second item


def test_sweep_layout():
    t = oc.SWEEP
    G = t.grid
    assert G == oc.OPT_GRID and 2 * G < t.items < 3 * G and t.chunks > 2 * oc.NPART
    got = oc.handoffs(t, G)
    assert oc.HANDOFFS <= got, oc.HANDOFFS - got
    # ragged last sweep: workgroup t.items - 2 G - 1 has a third item, the next one has none
    assert 0 < t.items - 2 * G < G
    assert sum(1 for e in t.entries if e.kind < 0) >= 2000 and all(e.numel <= 9 for e in t.entries if e.kind < 0)
    assert {e.numel for e in t.entries if e.kind < 0} == set(range(1, 10))
    # the clip-sum scratch is the head of the LDS that the first item of a workgroup overwrites: slab and parked row first
    assert {oc.item_class(t.of_item(i)) for i in range(G)} >= {"wide_row", "slab16", "slab32", "reg_row", "plain"}


def test_renorm_sweep_layout():
    assert oc.RENORM_SWEEP_ITEMS > 2 * oc.R_GRID
    paths = [oc.renorm_path(r, c, d) for (r, c), d in oc.RENORM_SWEEP]
    assert set(paths) == {"row_reg", "row_scalar", "panel64", "panel32"}
    scalar = {c for ((r, c), d), p in zip(oc.RENORM_SWEEP, paths) if p == "row_scalar"}
    assert {33, 50} <= scalar and any(c > oc.MAX_EMBD for c in scalar)


# ------------------------------------------------------------------------------------------------ fp32 inside, values
@pytest.mark.parametrize("name", list(oc.CASE_DEFS))
def test_fp32_restatements_inside_the_bounds(name):
    c, ref, bnd, vals = oc.oracle(name)
    for si in range(oc.NSTEPS):
        keys = oc.KEYS + (("norm",) if ref[si]["norm"] is not None else ())
        rc.close_values({k: vals[si][k] for k in keys}, bnd[si], ref[si], f"{name} step {si}")
    e32 = oc.adamw_eval(c.table, c.p0, c.steps, c.hyper, F32)
    oc.check_steps(e32, ref, bnd, f"cpu {name} torch sequence at fp32")
    w = oc.walk(c)
    oc.check_steps(w, ref, bnd, f"cpu {name} walk")
    assert oc.killed(name, None) is False
    if c.family == "exact":
        assert oc.norms_exact(w, c.steps) and oc.norms_exact(e32, c.steps)
        for si, (g32, mn) in enumerate(c.steps):
            assert float(ref[si]["norm"]) == pytest.approx(oc.exact_norm(g32), rel=1e-7)
    else:
        assert all(r["norm"] is None for r in ref)


def test_walk_does_not_depend_on_the_grid():
    """items are independent, and exact-sum partials add up exactly in any split: another grid, the same bits"""
    c = oc.case("edges_exact")
    a, b = oc.walk(c), oc.walk(c, grid=7, npart=5)
    for x, y in zip(a, b):
        assert x["norm"] == y["norm"]
        for k in oc.KEYS:
            assert rc.bits_equal(x[k], y[k])


def test_bounds_are_of_the_arithmetic():
    """plain (not normalised) entries: the bound of p after one step is some tens of fp32 roundings of |p| + |update|
    (|update| <= lr at step 1).  The largest single terms are the roundings of beta1 and beta2 to fp32, which 1 - beta
    magnifies by beta / (1 - beta): 9 and 19 / 2 roundings of the update."""
    c, ref, bnd, _ = oc.oracle("edges_gauss")
    for e in c.table.entries:
        if e.kind < 0:
            b = c.table.view(bnd[0]["p"], e)
            mag = c.table.view(ref[0]["p"], e).abs() + 2e-2
            assert (b <= 64 * rc.U32 * mag).all() and (b >= rc.U32 * c.table.view(ref[0]["p"], e).abs()).all()


# ------------------------------------------------------------------------------------------------ mutants
def test_kill_table_names_every_mutant():
    assert set(oc.KILLS) == set(oc.MUTANTS) and all(oc.KILLS[m] for m in oc.MUTANTS)
    assert all(n in oc.CASE_DEFS for ns in oc.KILLS.values() for n in ns)


@pytest.mark.parametrize("mutant", oc.MUTANTS)
def test_mutant_is_killed(mutant):
    """KILLS is the whole matrix: the named cases kill the mutant, the others do not (the clip mutants and the dropped
    chunk need clipping, the dropped last sweep a second sweep)"""
    for name in oc.CASE_DEFS:
        assert oc.killed(name, mutant) == (name in oc.KILLS[mutant]), (mutant, name)


def test_partial_chunk_is_shown_by_the_norm_alone():
    """one dropped chunk of 1 to 4204 elements among 300 k moves the clip factor by less than the bounds of most
    elements: the bit-exact norm is what shows it"""
    c = oc.case("edges_exact")
    assert not oc.norms_exact(oc.walk(c, mutant="partial_chunk_dropped"), c.steps)


# ------------------------------------------------------------------------------------------------ stand-alone renorm
@pytest.mark.parametrize("name", ["sweep", "edges"])
def test_renorm_fp32_inside(name):
    mats, ws, refs, bnds, vals = oc.renorm_oracle(name)
    worst = 0.0
    for (shape, d), w, ref, bnd, val in zip(mats, ws, refs, bnds, vals):
        rc.close_values({"o": val}, {"o": bnd}, {"o": ref}, f"renorm {shape} dim {d}")
        got = oc.renorm_eval(w, d, F32)
        worst = max(worst, oc.check(got, ref, bnd, f"cpu renorm {shape} dim {d}", verbose=False))
        nerr = (got.double().norm(dim=d) - 1).abs()
        assert (nerr <= oc.unit_norm_bound(ref, bnd, d)).all()
        # mutant: the norm over the other axis
        if min(shape) > 1:
            with pytest.raises(AssertionError):
                oc.check(oc.renorm_eval(w, 1 - d, F32), ref, bnd, "mutant", verbose=False)
    print(f"   cpu renorm {name}: max err/bound {worst:.3f}")
