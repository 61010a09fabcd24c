"""The oracles of kohonen_check.py have teeth (CPU only, no GPU): for every operation a straightforward fp32
restatement (the same torch math at float32) stays inside the bound at the shapes of the GPU tests, and one seeded
mutant - an emulation of a way the kernel can go wrong - falls outside it."""
import pytest
import torch

import gemm_check as gc
import kohonen_check as kc

F32 = torch.float32
G = 1.7   # upstream gradient of the scalar losses


def fails(fn):
    with pytest.raises(AssertionError):
        fn()


def quiet(got, ref, bound, label="mutant"):
    return lambda: kc.check_all(got, ref, bound, label, verbose=False)


# ------------------------------------------------------------------------------------------------ BMU
def bmu_fp32(x, nodes):
    """what the kernel computes: argmin of |n|^2 - 2 x.n in fp32."""
    return ((nodes * nodes).sum(-1)[None, :] - 2.0 * (x @ nodes.t())).argmin(dim=-1)


@pytest.mark.parametrize("M,N,C", kc.BMU_SHAPES)
def test_bmu_fp32_passes_and_wrong_rows_fail(M, N, C):
    x, nodes = gc.gauss_data((M, C), 1), gc.gauss_data((N, C), 2)
    idx = bmu_fp32(x, nodes)
    kc.bmu_check(idx, x, nodes, f"cpu bmu M{M} N{N} C{C}")
    bad = idx.clone()
    bad[M - 1] = (bad[M - 1] + 1) % N                           # the last (ragged) row takes a neighbour
    fails(lambda: kc.bmu_check(bad, x, nodes, "mutant", verbose=False))
    out = idx.clone()
    out[0] = 0x7FFFFFFF                                         # the "no comparison succeeded" value
    fails(lambda: kc.bmu_check(out, x, nodes, "mutant", verbose=False))


@pytest.mark.parametrize("N", [30, 256])
def test_bmu_tie_rule_first_minimum(N):
    x, nodes, want = kc.tie_case(N, 32, 3)
    q = (nodes * nodes).sum(-1)[None, :] - 2.0 * (x @ nodes.t())
    assert torch.equal(q.argmin(dim=-1), want)
    assert torch.equal(kc.bmu_ref(x, nodes), want)
    last = N - 1 - q.flip(-1).argmin(dim=-1)                    # last minimum wins
    assert not torch.equal(last, want) and (last > want).all()


def test_bmu_all_nan_row_reference_is_zero():
    x, nodes = gc.gauss_data((5, 32), 4), gc.gauss_data((9, 32), 5)
    x[2] = float("nan")
    assert kc.bmu_ref(x, nodes)[2].item() == 0


# ------------------------------------------------------------------------------------------------ scatter
@pytest.mark.parametrize("M,N,C", kc.SCATTER_FALLBACK + kc.SCATTER_GEMM)
def test_scatter_fp32_passes_and_mutants_fail(M, N, C):
    for name, idx in kc.index_patterns(M, N, 6).items():
        # integer data: exact
        d = gc.int_data((M, C), 4, 7)
        ref, _ = kc.scatter_ref(d, idx, N)
        gc.assert_exact(kc.scatter_fp32(d, idx, N), ref, f"scatter {name}")
        if name != "uniform":
            hit = torch.bincount(idx, minlength=N) > 0
            assert N == 1 or (~hit).any()
            assert (ref[~hit] == 0).all()
        keep = torch.ones(M, dtype=torch.bool)
        keep[M // 2] = False                                    # one dropped row
        dropped = kc.scatter_fp32(d[keep], idx[keep], N)
        if d[M // 2].abs().sum() > 0:
            fails(lambda: gc.assert_exact(dropped, ref, "mutant"))
        # Gaussian data: bound with n = hit count
        dg = gc.gauss_data((M, C), 8)
        ref, bound = kc.scatter_ref(dg, idx, N)
        kc.check(kc.scatter_fp32(dg, idx, N), ref, bound, f"cpu scatter {name} M{M} N{N} C{C}")
        fails(lambda: kc.check(kc.scatter_fp32(dg[keep], idx[keep], N), ref, bound, "mutant", verbose=False))
        if N > 1:                                               # a row credited to the next node
            moved = idx.clone()
            moved[M - 1] = (moved[M - 1] + 1) % N
            fails(lambda: kc.check(kc.scatter_fp32(dg, moved, N), ref, bound, "mutant", verbose=False))


# ------------------------------------------------------------------------------------------------ SOM update
@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("B,T,C,gm,gn", kc.SOM_UPDATE_SHAPES)
def test_som_update_fp32_passes_and_mutants_fail(B, T, C, gm, gn, periodic):
    from oracle import nvit_oracle as O
    nodes, x = gc.gauss_data((gm * gn, C), 9), gc.gauss_data((B, T, C), 10)
    idx = torch.randint(0, gm * gn, (B * T,), generator=torch.Generator().manual_seed(11))
    if B > 1:
        idx[1] = idx[0]                                         # two samples share a BMU
    sigma = (gm * gn) ** 0.5 / 2.0
    ref, bound = kc.som_update_eval(nodes, x, idx, 0.7 * 0.3, sigma, gm, gn, periodic)
    label = f"cpu som_update B{B} T{T} C{C} {gm}x{gn} periodic={periodic}"
    kc.check(kc.som_update_eval(nodes, x, idx, 0.7 * 0.3, sigma, gm, gn, periodic, dtype=F32)[0], ref, bound, label)
    # the oracle's literal restatement of the original loop, in fp32, is inside the bound as well
    lit = nodes.clone()
    O.som_update_(lit, x, idx, 0.7, 0.3, periodic)
    kc.check(lit, ref, bound, label + " (oracle loop)")
    if B > 1:       # batch-parallel instead of sequential: every sample applied to the ORIGINAL nodes
        par = nodes.clone()
        for i in range(B):
            one = kc.som_update_eval(nodes, x[i:i + 1], idx[i:i + 1], 0.7 * 0.3, sigma, gm, gn, periodic, dtype=F32)[0]
            par += one - nodes
        fails(lambda: kc.check(par, ref, bound, "mutant", verbose=False))
    if gm * gn > 1 and periodic:   # wrap-around ignored
        flat = kc.som_update_eval(nodes, x, idx, 0.7 * 0.3, sigma, gm, gn, False, dtype=F32)[0]
        fails(lambda: kc.check(flat, ref, bound, "mutant", verbose=False))
    if gm * gn == 1:               # strength without the learning rate
        fails(lambda: kc.check(kc.som_update_eval(nodes, x, idx, 0.3, sigma, gm, gn, periodic, dtype=F32)[0], ref,
                               bound, "mutant", verbose=False))


# ------------------------------------------------------------------------------------------------ consistency, huber
@pytest.mark.parametrize("M,C", kc.COS_SHAPES)
def test_cos_fp32_passes_and_mutants_fail(M, C):
    a, b = kc.cos_data(M, C, 12)
    ref, bound = kc.cos_eval(a, b, G), kc.cos_bounds(a, b, G)
    got = kc.cos_eval(a, b, G, dtype=F32)
    kc.check_all(got, ref, bound, f"cpu cos M{M} C{C}")
    # the last row left out of the sum (still divided by M); the gradient without 1/M... with M = 1 use a sign error
    cs_last = torch.nn.functional.cosine_similarity(a[-1:], b[-1:]).item()
    fails(quiet({**got, "loss": got["loss"] + cs_last / M}, ref, bound))
    fails(quiet({**got, "da": got["da"] * (M if M > 1 else -1)}, ref, bound))
    fails(quiet({**got, "db": got["da"]}, ref, bound))          # da written to both outputs


@pytest.mark.parametrize("n", kc.HUBER_SIZES)
def test_huber_fp32_passes_and_mutants_fail(n):
    a, b = kc.huber_data(n, 14)
    d = a.double() - b.double()
    assert (d == 1).any() and (d == -1).any() and (d == 0).any() and (d.abs() > 1).any() and (d.abs() < 1).any()
    ref, bound = kc.huber_eval(a, b, G), kc.huber_bounds(a, b, G)
    got = kc.huber_eval(a, b, G, dtype=F32)
    kc.check_all(got, ref, bound, f"cpu huber n{n}")
    mse = (0.5 * (a - b) ** 2).mean()                           # no linear branch
    fails(quiet({**got, "loss": mse}, ref, bound))
    fails(quiet({**got, "da": (a - b) * (G / n)}, ref, bound))  # gradient not clamped
    tail = got["da"].clone()
    tail[-4:] = 0                                               # the last vector of four never written
    fails(quiet({**got, "da": tail}, ref, bound))


# ------------------------------------------------------------------------------------------------ smoothness
@pytest.mark.parametrize("ms,C,M,pattern,dup", kc.SMOOTH_CASES)
def test_smooth_fp32_passes_and_mutants_fail(ms, C, M, pattern, dup):
    nodes = kc.smooth_nodes(ms, C, 15, dup)
    idx = kc.make_index(pattern, M, ms * ms, 16)
    if pattern == "wave":
        assert all(idx[i:i + 64].unique().numel() == 64 for i in range(0, M - 63, 64))
    ref, bound = kc.smooth_eval(nodes, idx, ms, G), kc.smooth_bounds(nodes, idx, ms, G)
    assert torch.isfinite(ref["dnodes"]).all()
    if dup:
        assert (ref["D"] == 0).any() and (bound["D"][ref["D"] == 0] == 0).all()
    got = kc.smooth_eval(nodes, idx, ms, G, dtype=F32, grouped=True)
    kc.check_all(got, ref, bound, f"cpu smooth ms{ms} C{C} M{M} {pattern} dup={dup}")
    assert torch.equal(got["cnt"], ref["cnt"])
    if ms >= 3:
        # neighbour (-1,-1) with the column offset's sign flipped: (-1,+1) twice, (-1,-1) never
        tab = kc.neighbour_table(ms)
        tab[:, 0] = tab[:, 2]
        bad = kc.smooth_eval(nodes, idx, ms, G, dtype=F32, table=tab, grouped=True)
        fails(quiet({k: bad[k] for k in ("D",)}, ref, {"D": bound["D"]}))
        fails(quiet({k: bad[k] for k in ("dnodes",)}, ref, {"dnodes": bound["dnodes"]}))
    if ms >= 2 and pattern != "one" and not (ms == 2 and dup):
        # only the "n as centre" half of the gradient: the pull of tokens on neighbouring nodes is lost
        nd = nodes.clone().requires_grad_(True)
        tabn = kc.neighbour_table(ms)
        dist = torch.linalg.vector_norm(nd[idx][:, None, :] - nd.detach()[tabn[idx]], dim=-1)
        (half,) = torch.autograd.grad(dist.mean(), nd, torch.tensor(G))
        fails(quiet({"dnodes": half}, ref, {"dnodes": bound["dnodes"]}))
    if ms >= 2:
        fails(quiet({"loss": got["loss"] * 8}, ref, {"loss": bound["loss"]}))   # mean over tokens only
    off = ref["cnt"].clone()
    off[ms * ms // 2] += 1                                      # one bin off by one
    assert not torch.equal(off, ref["cnt"])


# ------------------------------------------------------------------------------------------------ reconstruction
@pytest.mark.parametrize("B,ch,S,P", kc.RECON_SHAPES)
def test_recon_fp32_passes_and_mutants_fail(B, ch, S, P):
    raw, img = kc.recon_data(B, ch, S, P, 17)
    assert raw.abs().max().item() == 12.0
    ref, bound = kc.recon_eval(raw, img, P, G), kc.recon_bounds(raw, img, P, G)
    got = kc.recon_eval(raw, img, P, G, dtype=F32)
    kc.check_all(got, ref, bound, f"cpu recon B{B} ch{ch} S{S} P{P}")
    kc.check(got["draw"].bfloat16(), ref["draw"], bound["draw"], f"cpu recon bf16 B{B} ch{ch} S{S} P{P}")
    bad = kc.recon_eval(raw, img, P, G, dtype=F32, transpose_patch=True)   # ph and pw swapped
    fails(quiet(bad, ref, {"loss": bound["loss"]}))
    fails(quiet(bad, ref, {"draw": bound["draw"]}))
    trunc = (got["draw"].view(torch.int32) & -65536).view(F32).bfloat16()  # truncated, not rounded, to bf16
    fails(lambda: kc.check(trunc, ref["draw"], bound["draw"], "mutant", verbose=False))
    fails(quiet({**got, "draw": got["draw"] / 2}, ref, {"draw": bound["draw"]}))   # the 2 of d(x^2) missing


# ------------------------------------------------------------------------------------------------ pool + LayerNorm
def pool_data(B, T, C, seed=18):
    x = gc.gauss_data((B, T, C), seed) + 0.25
    w = 1 + 0.1 * gc.gauss_data((C,), seed + 1)
    b = 0.1 * gc.gauss_data((C,), seed + 2)
    g = gc.gauss_data((B, C), seed + 3)
    return x, w, b, g, gc.gauss_data((C,), seed + 4), gc.gauss_data((C,), seed + 5)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("B,T,C", kc.POOL_SHAPES)
def test_pool_ln_fp32_passes_and_mutants_fail(B, T, C, accumulate):
    x, w, b, g, odw, odb = pool_data(B, T, C)
    old = (odw, odb) if accumulate else (None, None)
    ref, bound = kc.pool_ln_eval(x, w, b, 1e-5, g, *old), kc.pool_ln_bounds(x, w, b, 1e-5, g, *old)
    got = kc.pool_ln_eval(x, w, b, 1e-5, g, *old, dtype=F32)
    kc.check_all(got, ref, bound, f"cpu pool_ln B{B} T{T} C{C} acc={accumulate}")
    if accumulate:      # `accumulate` ignored
        plain = kc.pool_ln_eval(x, w, b, 1e-5, g, dtype=F32)
        fails(quiet({**got, "dw": plain["dw"]}, ref, bound))
        fails(quiet({**got, "db": plain["db"]}, ref, bound))
    if T > 1:           # 1/T missing in dx; the last token left out of the pooled sum
        fails(quiet({**got, "dx": got["dx"] * T}, ref, bound))
        fails(quiet({**got, "pooled": x[:, :-1].sum(1) / T}, ref, bound))
    lo = got["ln"].bfloat16()
    trunc = (got["ln"].view(torch.int32) & -65536).view(F32).bfloat16()
    assert not gc.bits_equal(trunc, lo)                         # truncation differs from the one rounding bitwise
    fails(quiet({**got, "ln": got["ln"] - b}, ref, bound))      # bias dropped
    if C > 4:           # the last four columns left out of the mean over C
        short = torch.nn.functional.layer_norm(got["pooled"][:, :-4], (C - 4,), w[:-4], b[:-4], 1e-5)
        fails(quiet({**got, "ln": torch.cat([short, got["ln"][:, -4:]], dim=1)}, ref, bound))


# ------------------------------------------------------------------------------------------------ colsum / scale_cols
@pytest.mark.parametrize("with_b", [False, True])
@pytest.mark.parametrize("R,N,period", kc.COLSUM_CASES)
def test_colsum_scale_cols_fp32_pass_and_mutants_fail(R, N, period, with_b):
    a, b = gc.gauss_data((R, N), 24), (gc.gauss_data((R, N), 25) if with_b else None)
    old = gc.gauss_data((period, N), 26)
    for per, o in ((0, None), (period, None), (period, old)):
        P = max(per, 1)
        ref, bound = kc.colsum_ref(a, b, R, N, per, 0.5, None if o is None else o[:P])
        prod = a * b if with_b else a
        got = torch.zeros(P, N).index_add_(0, torch.arange(R) % P, prod) * 0.5
        if o is not None:
            got = got + o[:P]
        kc.check(got, ref, bound, f"cpu colsum R{R} N{N} period{per} b={with_b} acc={o is not None}")
        if R > 1:
            lost = torch.zeros(P, N).index_add_(0, torch.arange(R - 1) % P, prod[:-1]) * 0.5   # last row dropped
            fails(lambda: kc.check(lost + (0 if o is None else o[:P]), ref, bound, "mutant", verbose=False))
        if o is not None:
            fails(lambda: kc.check(got - o[:P], ref, bound, "mutant", verbose=False))          # `accumulate` ignored
    s = gc.gauss_data((N,), 27)
    ref, bound = kc.scale_cols_ref(a, s, 2.0)
    kc.check(a * s * 2.0, ref, bound, f"cpu scale_cols R{R} N{N}")
    kc.check((a * s * 2.0).bfloat16(), ref, bound, f"cpu scale_cols bf16 R{R} N{N}")
    fails(lambda: kc.check(a * s.roll(1) * 2.0, ref, bound, "mutant", verbose=False))          # column off by one
    trunc = ((a * s * 2.0).view(torch.int32) & -65536).view(F32).bfloat16()
    fails(lambda: kc.check(trunc, ref, bound, "mutant", verbose=False))
