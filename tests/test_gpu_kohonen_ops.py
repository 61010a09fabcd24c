"""GPU tests, op level: the Kohonen-head kernels (kohonen.hip), the pooled LayerNorm and the reconstruction loss
(misc.hip) and colsum / scale_cols against the fp64 references and error bounds of kohonen_check.py, at the edges of
their strides, chunkings and index patterns.  test_kohonen_check.py shows on the CPU that these bounds pass a correct
fp32 restatement and fail the mutants named there.  Run on the MI355X box: pytest -m gpu."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_check as gc
import kohonen_check as kc

G = 1.7   # upstream gradient of the scalar losses (not 1)


def dev():
    return torch.device("cuda:0")


def ops_():
    from nvit_amd import ops
    return ops


def gscalar():
    return torch.tensor(G, device=dev())


# ------------------------------------------------------------------------------------------------ BMU
@pytest.mark.parametrize("M,N,C", kc.BMU_SHAPES)
def test_som_bmu_vs_fp64_argmin(M, N, C):
    x, nodes = gc.gauss_data((M, C), 1), gc.gauss_data((N, C), 2)
    idx = ops_().som_bmu(x.to(dev()), nodes.to(dev()))
    kc.bmu_check(idx, x, nodes, f"som_bmu M{M} N{N} C{C}")


@pytest.mark.parametrize("N", [30, 256])
def test_som_bmu_ties_lowest_index_wins(N):
    """duplicated node rows in neighbouring lanes (5, 6), in one lane's strided loop (10, 74) and in far lanes
    (3, N-1): x equal to such a row must return the lower index."""
    x, nodes, want = kc.tie_case(N, 32, 3)
    filler = gc.gauss_data((5, 32), 4)                          # rows around the ties: a workgroup takes 4 rows
    xx = torch.cat([filler[:2], x, filler[2:]])
    idx = ops_().som_bmu(xx.to(dev()), nodes.to(dev())).cpu()
    assert ((idx >= 0) & (idx < N)).all()
    assert torch.equal(idx[2:2 + want.numel()], want), (idx, want)
    assert torch.equal(idx, kc.bmu_ref(xx, nodes))


def test_som_bmu_all_nan_row_returns_index_zero():
    """every distance of an all-NaN row is NaN: torch.argmin of the reference gives 0, and no index may leave [0, N)
    (it becomes a row number in gather_rows).  som_bmu only: nothing is gathered here."""
    for M, N, C in [(9, 30, 32), (70, 256, 64)]:
        x, nodes = gc.gauss_data((M, C), 5), gc.gauss_data((N, C), 6)
        x[3] = float("nan")
        x[M - 1] = float("nan")
        idx = ops_().som_bmu(x.to(dev()), nodes.to(dev())).cpu()
        assert ((idx >= 0) & (idx < N)).all(), idx
        ref = kc.bmu_ref(x, nodes)
        assert ref[3].item() == 0 and idx[3].item() == 0 and idx[M - 1].item() == 0
        assert torch.equal(idx, ref)


# ------------------------------------------------------------------------------------------------ gather / onehot
@pytest.mark.parametrize("M,C", kc.GATHER_SHAPES)
def test_gather_rows_bit_exact(M, C):
    nodes = gc.gauss_data((36, C), 7)
    idx = torch.randint(0, 36, (M,), generator=torch.Generator().manual_seed(8))
    idx[0], idx[-1] = 35, 0
    out = ops_().gather_rows(nodes.to(dev()), idx.to(dev())).cpu()
    assert gc.bits_equal(out, nodes[idx])


@pytest.mark.parametrize("N", kc.ONEHOT_N)
def test_onehot_bit_exact(N):
    for M in (1, 1001):
        idx = torch.randint(0, N, (M,), generator=torch.Generator().manual_seed(9))
        idx[0] = N - 1
        oh = ops_().onehot(idx.to(dev()), N)
        assert gc.bits_equal(oh.cpu(), torch.nn.functional.one_hot(idx, N).float())


# ------------------------------------------------------------------------------------------------ scatter
@pytest.mark.parametrize("M,N,C", kc.SCATTER_FALLBACK + kc.SCATTER_GEMM)
def test_scatter_rows_exact_and_bounded(M, N, C):
    """both routes of ops.scatter_rows (the ballot kernel for N % 4 or C % 4 != 0, one-hot + TN GEMM otherwise):
    integer data bit-identical to the fp64 index_add_, empty nodes exactly 0, Gaussian data inside the bound."""
    ops = ops_()
    assert (N % 4 != 0 or C % 4 != 0) == ((M, N, C) in kc.SCATTER_FALLBACK)
    for name, idx in kc.index_patterns(M, N, 6).items():
        d = gc.int_data((M, C), 4, 7)
        ref, _ = kc.scatter_ref(d, idx, N)
        out = ops.scatter_rows(d.to(dev()), idx.to(dev()), N).cpu()
        gc.assert_exact(out, ref, f"scatter_rows {name} M{M} N{N} C{C}")
        empty = torch.bincount(idx, minlength=N) == 0
        assert (out[empty] == 0).all()
        dg = gc.gauss_data((M, C), 8)
        ref, bound = kc.scatter_ref(dg, idx, N)
        kc.check(ops.scatter_rows(dg.to(dev()), idx.to(dev()), N), ref, bound, f"scatter_rows {name} M{M} N{N} C{C}")


@pytest.mark.parametrize("N", [30, 36])
def test_kohonen_map_forward_backward_node_gradient(N):
    """KohonenMap.forward(x)[0].backward(g): nodes.grad = index_add_ of g by the winning index (N = 30: the ballot
    kernel, N = 36: the one-hot GEMM)."""
    from nvit_amd.kohonen import KohonenMap
    M, C = 1001, 64
    torch.manual_seed(10)
    km = KohonenMap(C, N).to(dev())
    x, g = gc.gauss_data((M, C), 11), gc.gauss_data((M, C), 12)
    nodes = km.nodes.detach().cpu().clone()
    out, idx = km(x.to(dev()))
    kc.bmu_check(idx, x, nodes, f"KohonenMap N{N} forward")
    idx = idx.cpu()
    assert torch.bincount(idx, minlength=N).gt(0).sum().item() > N // 2      # a spread histogram
    assert gc.bits_equal(out.detach().cpu(), nodes[idx])
    out.backward(g.to(dev()))
    ref, bound = kc.scatter_ref(g, idx, N)
    kc.check(km.nodes.grad, ref, bound, f"KohonenMap N{N} nodes.grad")


# ------------------------------------------------------------------------------------------------ SOM update
@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("B,T,C,gm,gn", kc.SOM_UPDATE_SHAPES)
def test_som_update_vs_fp64_sequential(B, T, C, gm, gn, periodic):
    nodes, x = gc.gauss_data((gm * gn, C), 9), gc.gauss_data((B, T, C), 10)
    idx = torch.randint(0, gm * gn, (B * T,), generator=torch.Generator().manual_seed(11))
    if B > 1:
        idx[1] = idx[0]                                         # two samples share a BMU
    sigma = (gm * gn) ** 0.5 / 2.0
    ref, bound = kc.som_update_eval(nodes, x, idx, 0.7 * 0.3, sigma, gm, gn, periodic)
    nd = nodes.to(dev())
    ops_().som_update(nd, x.to(dev()), idx.to(dev()), 0.7 * 0.3, sigma, gm, gn, B, T, periodic=periodic)
    kc.check(nd, ref, bound, f"som_update B{B} T{T} C{C} {gm}x{gn} periodic={periodic}")


# ------------------------------------------------------------------------------------------------ consistency, huber
@pytest.mark.parametrize("M,C", kc.COS_SHAPES)
def test_cos_consistency_fwd_bwd(M, C):
    from nvit_amd.kohonen import CosConsistencyFn
    a, b = kc.cos_data(M, C, 12)
    ad, bd = a.to(dev()).requires_grad_(True), b.to(dev()).requires_grad_(True)
    loss = CosConsistencyFn.apply(ad, bd)
    loss.backward(gscalar())
    kc.check_all({"loss": loss, "da": ad.grad, "db": bd.grad}, kc.cos_eval(a, b, G), kc.cos_bounds(a, b, G),
                 f"cos_consistency M{M} C{C}")


@pytest.mark.parametrize("n", kc.HUBER_SIZES)
def test_huber_fwd_bwd(n):
    from nvit_amd.kohonen import HuberFn
    a, b = kc.huber_data(n, 14)
    ad, bd = a.to(dev()).requires_grad_(True), b.to(dev()).requires_grad_(True)
    loss = HuberFn.apply(ad, bd)
    loss.backward(gscalar())
    kc.check_all({"loss": loss, "da": ad.grad, "db": bd.grad}, kc.huber_eval(a, b, G), kc.huber_bounds(a, b, G),
                 f"huber n{n}")


# ------------------------------------------------------------------------------------------------ smoothness
@pytest.mark.parametrize("ms,C,M,pattern,dup", kc.SMOOTH_CASES)
def test_som_smooth_fwd_bwd(ms, C, M, pattern, dup):
    from nvit_amd.kohonen import MapSmoothnessFn
    nodes = kc.smooth_nodes(ms, C, 15, dup)
    idx = kc.make_index(pattern, M, ms * ms, 16)
    ref, bound = kc.smooth_eval(nodes, idx, ms, G), kc.smooth_bounds(nodes, idx, ms, G)
    assert torch.isfinite(ref["dnodes"]).all()
    _, cnt, D = ops_().som_smooth_fwd(nodes.to(dev()), idx.to(dev()), ms)
    assert torch.equal(cnt.cpu().long(), ref["cnt"]), "histogram differs from torch.bincount"
    nd = nodes.to(dev()).requires_grad_(True)
    loss = MapSmoothnessFn.apply(nd, idx.to(dev()), ms)
    loss.backward(gscalar())
    kc.check_all({"loss": loss, "D": D, "dnodes": nd.grad}, ref, bound,
                 f"som_smooth ms{ms} C{C} M{M} {pattern} dup={dup}")


# ------------------------------------------------------------------------------------------------ reconstruction
@pytest.mark.parametrize("B,ch,S,P", kc.RECON_SHAPES)
def test_recon_loss_and_bwd(B, ch, S, P):
    from nvit_amd._lib import BF16, F32
    ops = ops_()
    raw, img = kc.recon_data(B, ch, S, P, 17)
    ref, bound = kc.recon_eval(raw, img, P, G), kc.recon_bounds(raw, img, P, G)
    rd, im = raw.to(dev()), img.to(dev())
    label = f"recon B{B} ch{ch} S{S} P{P}"
    kc.check(ops.recon_loss(rd, im, P), ref["loss"], bound["loss"], label + " loss")
    g1 = gscalar().reshape(1)
    for dt, name in ((F32, "fp32"), (BF16, "bf16")):
        draw = ops.recon_bwd(dt, rd, im, g1, P)
        assert draw.dtype == ops.tdtype(dt)
        kc.check(draw, ref["draw"], bound["draw"], f"{label} draw {name}")


# ------------------------------------------------------------------------------------------------ pool + LayerNorm
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("dt_name", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T,C", kc.POOL_SHAPES)
def test_pool_ln_fwd_bwd(B, T, C, dt_name, accumulate):
    from nvit_amd import _lib
    ops = ops_()
    dt = _lib.F32 if dt_name == "fp32" else _lib.BF16
    d = dev()
    x = gc.gauss_data((B, T, C), 18) + 0.25
    w, b = 1 + 0.1 * gc.gauss_data((C,), 19), 0.1 * gc.gauss_data((C,), 20)
    g = gc.gauss_data((B, C), 21)
    odw, odb = gc.gauss_data((C,), 22), gc.gauss_data((C,), 23)
    old = (odw, odb) if accumulate else (None, None)
    ref, bound = kc.pool_ln_eval(x, w, b, 1e-5, g, *old), kc.pool_ln_bounds(x, w, b, 1e-5, g, *old)
    pooled, ln, ln_lo, stats = ops.pool_ln_fwd(dt, x.reshape(B * T, C).to(d), w.to(d), b.to(d), 1e-5, B, T, C)
    assert ln_lo.dtype == ops.tdtype(dt)
    assert gc.bits_equal(ln_lo.cpu(), ln.cpu().to(ops.tdtype(dt))), "ln_lo is not ONE rounding of ln"
    dw = odw.to(d) if accumulate else torch.full((C,), float("nan"), device=d)
    db = odb.to(d) if accumulate else torch.full((C,), float("nan"), device=d)
    dx = ops.pool_ln_bwd(g.to(d), pooled, w.to(d), stats, dw, db, accumulate, B, T, C)
    kc.check_all({"pooled": pooled, "ln": ln, "dx": dx.reshape(B, T, C), "dw": dw, "db": db}, ref, bound,
                 f"pool_ln B{B} T{T} C{C} {dt_name} acc={accumulate}")


# ------------------------------------------------------------------------------------------------ colsum / scale_cols
@pytest.mark.parametrize("in_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("with_b", [False, True])
@pytest.mark.parametrize("R,N,period", kc.COLSUM_CASES)
def test_colsum_bounded_and_exact(R, N, period, with_b, in_dtype):
    ops = ops_()
    d = dev()
    a = gc.gauss_data((R, N), 24).to(in_dtype)
    b = gc.gauss_data((R, N), 25).to(in_dtype) if with_b else None
    old = gc.gauss_data((period, N), 26)
    bd = b.to(d) if with_b else None
    for per, o in ((0, None), (period, None), (period, old)):
        P = max(per, 1)
        ref, bound = kc.colsum_ref(a, b, R, N, per, 0.5, None if o is None else o[:P])
        out = o[:P].clone().to(d) if o is not None else torch.full((P, N), float("nan"), device=d)
        ops.colsum(a.to(d), R, N, out, o is not None, b=bd, period=per, scale=0.5)
        kc.check(out, ref, bound, f"colsum R{R} N{N} period{per} b={with_b} {in_dtype} acc={o is not None}")
    # small integers, power-of-two scale: exact
    ai = gc.int_data((R, N), 4, 27).to(in_dtype)
    bi = gc.int_data((R, N), 4, 28).to(in_dtype) if with_b else None
    oi = gc.int_data((period, N), 16, 29)
    ref, _ = kc.colsum_ref(ai, bi, R, N, period, 2.0, oi)
    out = oi.clone().to(d)
    ops.colsum(ai.to(d), R, N, out, True, b=bi.to(d) if with_b else None, period=period, scale=2.0)
    gc.assert_exact(out.cpu(), ref, f"colsum exact R{R} N{N}")


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("R,N,period", kc.COLSUM_CASES)
def test_scale_cols_bounded_and_exact(R, N, period, out_dtype):
    ops = ops_()
    d = dev()
    a, s = gc.gauss_data((R, N), 24), gc.gauss_data((N,), 27)
    ref, bound = kc.scale_cols_ref(a, s, 2.0)
    out = ops.scale_cols(a.to(d), s.to(d), 2.0, R, N, torch.empty((R, N), device=d, dtype=out_dtype))
    kc.check(out, ref, bound, f"scale_cols R{R} N{N} {out_dtype}")
    ai, si = gc.int_data((R, N), 64, 30), gc.pow2_data(N, 31)
    ref, _ = kc.scale_cols_ref(ai, si, 0.5)
    out = ops.scale_cols(ai.to(d), si.to(d), 0.5, R, N, torch.empty((R, N), device=d, dtype=out_dtype))
    gc.assert_exact(out.cpu(), ref, f"scale_cols exact R{R} N{N} {out_dtype}")
