"""GPU: the fused optimizer step (grad_sqnorm_kernel, adamw_renorm_kernel plain and skip_nonfinite) and the stand-alone
renorm_kernel, element by element against the fp64 reference and the derived bounds of tests/optim_check.py.

Every element of p, exp_avg and exp_avg_sq of every table entry is compared after each of three steps, through
FusedAdamW.step_fused with three param groups and one lr rewritten between two steps.  EDGES is one sweep with an entry
per geometric edge; SWEEP makes every workgroup of both grids take a second item and some a third, with the LDS
hand-offs between consecutive items that optim_check asserts.  All inputs are finite and inside the documented ranges.
"""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import optim_check as oc
import rowops_check as rc

DEV = "cuda:0"


def run_fused(c: oc.Case, skip_nonfinite: bool = False):
    """the steps of case c through FusedAdamW.step_fused -> [{p, m, v (flat, CPU), norm}] as optim_check.adamw_eval.
    p, g, exp_avg and exp_avg_sq of all entries live in one device vector each (the layout of optim_check.Table)."""
    from nvit_amd.optim import FusedAdamW
    t = c.table
    flat = {k: torch.zeros(t.total, device=DEV) for k in "pgmv"}
    flat["p"].copy_(c.p0)
    view = lambda k, e: flat[k][e.off:e.off + e.numel].view(e.shape)
    params = [torch.nn.Parameter(view("p", e)) for e in t.entries]
    groups = [{"params": [p for p, e in zip(params, t.entries) if e.group == gi], **g}
              for gi, g in enumerate(c.hyper["groups"])]
    assert all(g["params"] for g in groups)
    opt = FusedAdamW(groups, lr=1e-3, betas=c.hyper["betas"], eps=c.hyper["eps"])
    for p, e in zip(params, t.entries):
        assert p.data_ptr() == flat["p"].data_ptr() + 4 * e.off and p.data_ptr() % 16 == 0
        p.grad = view("g", e)
        opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": view("m", e), "exp_avg_sq": view("v", e)}
    model = oc._fake_model([p for p, e in zip(params, t.entries) if e.kind == 1],
                           [p for p, e in zip(params, t.entries) if e.kind == 0])
    at, gi, lr = c.hyper["lr_change"]
    out, table = [], None
    for si, (g32, max_norm) in enumerate(c.steps):
        if si == at:
            opt.param_groups[gi]["lr"] = lr
        flat["g"].copy_(g32)
        gn = opt.step_fused(model, max_norm, skip_nonfinite=skip_nonfinite)
        cache = opt._cache
        assert (cache["n"], cache["items"], cache["chunks"]) == (len(t.entries), t.items, t.chunks)
        table = cache["table"] if table is None else table
        assert cache["table"] is table, "the lr change must take the in-place hyper-column rewrite, not a rebuild"
        assert (gn is not None) == (max_norm > 0 or skip_nonfinite)
        out.append({"p": flat["p"].cpu(), "m": flat["m"].cpu(), "v": flat["v"].cpu(),
                    "norm": None if max_norm <= 0 else gn.item()})
    torch.cuda.synchronize()
    if skip_nonfinite:
        assert opt.skipped_steps() == 0
    assert float(opt.state_dict()["state"][0]["step"]) == float(len(c.steps))
    return out


def fused_case(name: str):
    t0 = time.perf_counter()
    c, ref, bnd, _ = oc.oracle(name)
    t1 = time.perf_counter()
    got = run_fused(c)
    worst = oc.check_steps(got, ref, bnd, f"gpu {name}")
    print(f"   gpu {name}: oracle {t1 - t0:.2f} s, GPU steps and checks {time.perf_counter() - t1:.2f} s")
    return c, got, worst


def test_edges_gauss_unclipped():
    """EDGES, Gaussian gradients of three magnitudes with near-eps and zero elements, grad_clip = 0"""
    c, got, _ = fused_case("edges_gauss")
    assert all(g["norm"] is None for g in got)


def test_edges_exact_clipped():
    """EDGES, exact-sum gradients: a clipped step, one with the factor exactly 1, a tiny clipped one; bit-exact norm"""
    c, got, _ = fused_case("edges_exact")
    assert oc.norms_exact(got, c.steps), [g["norm"] for g in got]


def test_sweep_exact_clipped_and_guarded_twin():
    """SWEEP: two full sweeps and a ragged third of the update grid, more than two of the norm grid; the norm bit-exact at
    every step; the skip_nonfinite instantiation gives the same bits of p, m, v and norm"""
    c, got, _ = fused_case("sweep")
    assert oc.norms_exact(got, c.steps), [g["norm"] for g in got]
    t0 = time.perf_counter()
    twin = run_fused(c, skip_nonfinite=True)
    for si, (a, b) in enumerate(zip(got, twin)):
        assert a["norm"] == b["norm"], (si, a["norm"], b["norm"])
        for k in oc.KEYS:
            assert rc.bits_equal(a[k], b[k]), (si, k)
    print(f"   gpu sweep guarded twin: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("name", ["sweep", "edges"])
def test_renorm_kernel(name):
    """ops.renorm_table / ops.renorm_weights, all matrices of the list in one launch: every element inside the fp64 bound,
    every normalised row / column norm within its bound of 1"""
    from nvit_amd import ops
    t0 = time.perf_counter()
    mats, ws, refs, bnds, _ = oc.renorm_oracle(name)
    t1 = time.perf_counter()
    dws = [w.to(DEV).contiguous() for w in ws]
    table, items = ops.renorm_table([(dw, d) for dw, (_, d) in zip(dws, mats)], torch.device(DEV))
    assert items == sum(oc.renorm_items(r, c, d) for (r, c), d in mats)
    ops.renorm_weights(table, items)
    worst = worst_n = 0.0
    for (shape, d), dw, ref, bnd in zip(mats, dws, refs, bnds):
        got = dw.cpu()
        worst = max(worst, oc.check(got, ref, bnd, f"gpu renorm {shape} dim {d}", verbose=False))
        nerr = (got.double().norm(dim=d) - 1).abs()
        nb = oc.unit_norm_bound(ref, bnd, d)
        assert (nerr <= nb).all(), (shape, d, (nerr / nb).max().item())
        worst_n = max(worst_n, (nerr / nb).max().item())
    print(f"   gpu renorm {name}: max err/bound element {worst:.3f} unit norm {worst_n:.3f}; "
          f"oracle {t1 - t0:.2f} s, GPU and checks {time.perf_counter() - t1:.2f} s")
