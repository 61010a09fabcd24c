"""The oracles of epilogue_check.py have teeth (CPU only, no GPU): at every shape of test_gpu_epilogue_bounds.py an fp32
evaluation of each reference - with expf and a division, and with the epilogues' exp2(fl(x * fl(log2 e))) - stays inside
its bound, a bf16 rounding of it stays inside the bound + half an ulp, every case passes require_exact, and the mutants -
one-line variants of the references, the ways these epilogues can go wrong - fall outside."""
import math

import pytest
import torch

import epilogue_check as ec
import gemm_check as gc
import rowops_check as rc

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
PRESCALE = math.sqrt(64) * 1.4426950408889634     # ops.attn_q_prescale(64) (the package needs the built library)
N_CU = 256


def fails(fn):
    with pytest.raises(AssertionError):
        fn()


MUTANTS = {}        # "launch mutant" -> the smallest err / bound it reached over the shapes of this run (printed with -s)


def outside(tag, got, ref, bound, also_bf16=True):
    """the mutant's value, and its bf16 rounding, leave the bound (an exact output: its bf16 rounding has other bits)"""
    if bound is None:
        got = got.bfloat16()
    forms = [got] + ([got.bfloat16()] if also_bf16 and bound is not None else [])
    for g in forms:
        fails(lambda: ec.check_or_exact(g, ref, bound, "mutant", verbose=False))
        m = ec.margin(g, ref, bound)
        assert m > 1.0
        MUTANTS[tag] = min(MUTANTS.get(tag, math.inf), m)


def report(launch):
    for tag, m in sorted(MUTANTS.items()):
        if tag.startswith(launch):
            print(f"== mutant {tag}: smallest err/bound {m:.3g}")


def swiglu_cases(M):
    for F, K in ec.SWIGLU_FK:
        for gs in (True, False):
            yield F, K, gs, False
    for launch, (Mb, F, K, gs) in ec.SWIGLU_BIAS.items():
        if Mb == M:
            yield F, K, gs, True


# ------------------------------------------------------------------------------------------------ the exponential
def test_fast_exp_needs_and_keeps_the_derived_allowance():
    """exp2(fl(x * fl(log2 e))) in fp32 against exp in fp64: beyond the flat LIB roundings of expf from |x| of a few on,
    inside (2 |x| + 2) roundings everywhere"""
    x = torch.linspace(-30.0, 30.0, 200001, dtype=F32)
    got = ec._fast_exp(x)
    assert got.dtype == F32
    want = torch.exp(x.double())
    roundings = (got.double() - want).abs() / want / rc.U32
    allowed = 2.0 * x.double().abs() + 2.0
    assert (roundings <= allowed).all()
    near7 = (x.abs() > 6.5) & (x.abs() < 7.5)
    assert roundings[near7].max() > rc.LIB, "the flat allowance would do: the derivation is not needed"
    assert roundings[near7].max() < 16.0
    ev = ec._fast_exp(rc.Ev(x))
    assert torch.allclose(ev.e, want * allowed * rc.U32 + ec.FTZ, rtol=1e-12, atol=0.0)
    with ec.fast_math():
        assert rc._exp is ec._fast_exp and rc._recip is ec._fast_recip
    assert rc._exp is not ec._fast_exp and rc._recip is not ec._fast_recip


# ------------------------------------------------------------------------------------------------ EPI 3 / 6
@pytest.mark.parametrize("M", ec.EDGE_M)
def test_swiglu_fwd_fp32_inside_and_mutants_outside(M):
    for F, K, gs, bias in swiglu_cases(M):
        d = ec.swiglu_fwd_case(M, F, K, 11, gs, bias)
        c = ec.swiglu_fwd_c(d)
        label = f"EPI3 M{M} F{F} K{K} gs={gs} bias={bias}"
        ref, bnd = ec.swiglu_fwd_ref(c)
        with ec.fast_math():
            vals, _ = rc.swiglu_bounds(c)
        rc.close_values({"x": vals["x"]}, {"x": bnd}, {"x": ref}, label)
        for fast in (False, True):
            got = ec.swiglu_fwd_f32(c, fast)
            m32 = rc.check(got, ref, bnd, f"cpu {label} fp32 fast={fast}")
            rc.check(got.bfloat16(), ref, bnd, f"cpu {label} bf16 fast={fast}", verbose=False)
            # what shows through the bf16 rounding is a lower estimate of the fp32 margin
            assert ec.crossed(got.bfloat16(), ref, bnd) <= m32 * (1 + 1e-6)
            assert ec.misrounded(got.bfloat16(), ref) < 0.05 and ec.crossed(ref.float().bfloat16(), ref, bnd) == 0.0
        gc.assert_exact(ec.round_bf16(c["acc"]), c["acc"], label + " uv")
        for kind in ("partner", "sign"):
            outside(f"EPI3/6 x {kind}", ec.swiglu_fwd_mutant(c, kind), ref, bnd)
        if K == 320 and M > 1:      # the planted sums leave bf16's 8 bits: a truncated raw tile shows
            fails(lambda: gc.assert_exact(ec.trunc_bf16(c["acc"]), c["acc"], "mutant"))
    report("EPI3")


def test_interleaved_vectors_are_the_kernels_order():
    F = 128
    gs = gc.gauss_data((2 * F,), 3)
    assert torch.equal(ec.interleave(gs, F)[gc.perm_rows(2 * F).argsort()], gs)
    assert torch.equal(ec.deinterleave(ec.interleave(gs, F), F), gs)


# ------------------------------------------------------------------------------------------------ EPI 5
@pytest.mark.parametrize("M", ec.EDGE_M)
def test_swiglu_bwd_fp32_inside_and_mutants_outside(M):
    for F, K in ec.BWD_FK:
        for gs in (True, False):
            d = ec.swiglu_bwd_case(M, F, K, 21, gs)
            c = ec.swiglu_bwd_c(d)
            label = f"EPI5 M{M} F{F} K{K} gs={gs}"
            ref, bnd = ec.swiglu_bwd_ref(c)
            assert set(ref) == ({"duv", "part", "dsuv"} if gs else {"duv"})
            for fast in (False, True):
                got = ec.swiglu_bwd_f32(c, fast)
                rc.check(got["duv"], ref["duv"], bnd["duv"], f"cpu {label} duv fast={fast}")
                rc.check(got["duv"].bfloat16(), ref["duv"], bnd["duv"], f"cpu {label} duv bf16", verbose=False)
                if gs:
                    rc.check(got["part"], ref["part"], bnd["part"], f"cpu {label} part fast={fast}")
                    rc.check(got["dsuv"], ref["dsuv"], bnd["dsuv"] + rc.csr_bound(got["part"]),
                             f"cpu {label} dsuv fast={fast}")
            outside("EPI5 duv dv_mutant", rc.swiglu_eval(c, dv_mutant=True)["duv"], ref["duv"], bnd["duv"])
            trunc = ec.swiglu_bwd_c(d, dx_of=ec.trunc_bf16)
            differ = (trunc["dx"] != c["dx"]).sum().item()
            if K == 320 and M > 1:
                assert differ > 0
            if differ:
                outside("EPI5 duv dx truncated", rc.swiglu_eval(trunc)["duv"], ref["duv"], bnd["duv"])
            if not gs:
                continue
            nblk = ec.part_blocks(M)
            assert ref["part"].shape == (nblk, 2 * F) and nblk == (2 if M <= 256 else 4)
            live = -(-M // ec.PART_ROWS)
            assert (ref["part"][live:] == 0).all() and (bnd["part"][live:] == 0).all()
            assert (bnd["part"][:live] > 0).any(1).all()      # (a zero dx leaves a zero term with a zero bound)
            # the block sums are the autograd reference's d(suv), split by rows
            tol = 1e-12 * rc.swiglu_eval(c)["dsuv_rows"].abs().sum(0)
            assert ((ref["part"].sum(0) - ref["dsuv"]).abs() <= tol).all()
            for kind in ("dead", "shift"):
                mut, _ = ec.swiglu_bwd_ref(c, mutant=kind)
                outside(f"EPI5 part {kind}", mut["part"], ref["part"], bnd["part"], also_bf16=False)
            nan_left = ref["part"].clone()
            nan_left[-1, 5] = float("nan")      # a dead row left unwritten in the NaN-filled buffer
            fails(lambda: rc.check(nan_left, ref["part"], bnd["part"], "mutant", verbose=False))
    report("EPI5")


# ------------------------------------------------------------------------------------------------ EPI 4
@pytest.mark.parametrize("case", ec.QK_CASES, ids=ec.qk_id)
def test_qk_fused_fp32_inside_and_mutants_outside(case):
    Bsz, T, H, K, nparts, part0, norm, bias = case
    d = ec.qk_fused_case(Bsz, T, H, K, nparts, part0, 31, norm, bias)
    c = ec.qk_fused_c(d)
    label = "EPI4 " + ec.qk_id(case)
    ref, bnd = ec.qk_fused_ref(c, PRESCALE)
    have = set(range(part0, part0 + nparts))
    want = {n + "h" for p, n in enumerate("qkv") if p in have}
    if norm:
        want |= {"r" + n for p, n in enumerate("qk") if p in have}
    assert set(ref) == want
    exact = {k for k in ref if bnd[k] is None}
    assert exact == ({"vh"} if norm else {"kh", "vh"}) & want
    got = ec.qk_fused_f32(c, PRESCALE)
    assert set(got) == want - exact
    for k in got:
        rc.check(got[k], ref[k], bnd[k], f"cpu {label} {k} fp32")
        if k.endswith("h"):
            rc.check(got[k].bfloat16(), ref[k], bnd[k], f"cpu {label} {k} bf16", verbose=False)
    for k in exact:
        gc.assert_exact(ec.round_bf16(ref[k]), ref[k], label)
    # q as stored: un-scaling it is not what is checked
    if norm and 0 in have:
        fails(lambda: rc.check(got["qh"] / PRESCALE, ref["qh"], bnd["qh"], "mutant", verbose=False))
        once = rc.qknorm_fwd_formula(dict(c, c_q=c["c_q"] * PRESCALE), "ev")["qh"].e    # one constant, rounded once
        assert (bnd["qh"] >= once).all() and (bnd["qh"] > once)[ref["qh"] != 0].all(), \
            "the extra rounding of the folded constant is not carried"
    # ---- mutants
    if norm and have & {0, 1}:
        for kind in ("group32", "group128"):
            mut = ec.qk_fused_mutant(c, PRESCALE, kind)
            for k in ("qh", "kh"):
                if k in ref:
                    outside(f"EPI4 {k} {kind}", mut[k], ref[k], bnd[k])
        if 1 in have:
            outside("EPI4 kh prescale_k", ec.qk_fused_mutant(c, PRESCALE, "prescale_k")["kh"], ref["kh"], bnd["kh"])
        if bias:
            mut = ec.qk_fused_mutant(c, PRESCALE, "bias_late", d["bias"], part0)
            for k in mut:
                outside(f"EPI4 {k} bias_late", mut[k], ref[k], bnd[k])
    # ---- the head split: rows placed with too few wraps into the next batch
    flat = {"qh": 0, "kh": 1, "vh": 2}
    for k in want & set(flat):
        rows = rc.from_heads(ref[k], Bsz, T, H, ec.HEAD)
        assert torch.equal(ec.head_scatter(rows, Bsz, T, H), ref[k])
        for wraps in (0, 1):
            crossings = (min(ec.WAVE_ROWS, Bsz * T) - 1) // T      # batch crossings inside the first wave tile
            mut = ec.head_scatter(rows, Bsz, T, H, wraps)
            if crossings > wraps or (wraps == 0 and Bsz * T > ec.WAVE_ROWS and Bsz > 1):
                outside(f"EPI4 head split, {wraps} wraps", mut, ref[k], bnd[k], also_bf16=False)
            elif Bsz == 1:
                assert torch.equal(mut, ref[k])
    report("EPI4")


# ------------------------------------------------------------------------------------------------ many rounds
def test_rounds_shapes():
    assert ec.rounds_shape(N_CU) == (144 * 256 + 37, 64 * 256)
    assert ec.rounds_shape(N_CU, 256) == (144 * 256, 64 * 256)
    M, sl = ec.rounds_shape(N_CU, ec.ROUNDS_QK_T)
    assert (M, sl) == (36889, 9472) and M % ec.ROUNDS_QK_T == 0 and M % 256 == 25
    for n in (64, 256, 304):
        for T in (None, 256, ec.ROUNDS_QK_T):
            if T == ec.ROUNDS_QK_T and n < 37 * 4:      # (a slice of whole tiles and whole batches is 37 row tiles)
                continue
            M, sl = ec.rounds_shape(n, T)
            tiles = -(-M // 256) * 4
            assert 2.0 * n <= tiles <= 2.5 * n and sl % 256 == 0 and sl // 256 * 4 <= n
            assert T is None or (M % T == 0 and sl % T == 0)
            assert T == 256 or M % 256
    for K, _ in ec.ROUNDS_K:
        gc.require_exact(K, 2, 2, pre_scale=8)


def test_rounds_sampled_rows_inside():
    """the rows the many-rounds GPU cases hold against the bounds, at K = 384"""
    K = 384
    M, _ = ec.rounds_shape(N_CU)
    rows = gc.sample_rows(M)
    assert rows is not None and len(rows) < 1000
    d = ec.swiglu_fwd_case(M, 512, K, 41)
    c = ec.swiglu_fwd_c(d, rows)
    ref, bnd = ec.swiglu_fwd_ref(c)
    rc.check(ec.swiglu_fwd_f32(c, True), ref, bnd, "cpu rounds EPI3 x")
    d = ec.swiglu_bwd_case(M, 1024, K, 42)
    c = ec.swiglu_bwd_c(d, rows)
    ref, bnd = ec.swiglu_bwd_ref(c, nblk=ec.part_blocks(len(rows)))
    rc.check(ec.swiglu_bwd_f32(c, True)["duv"], ref["duv"], bnd["duv"], "cpu rounds EPI5 duv")
    last = torch.arange((M - 1) // 256 * 256, M)
    c = ec.swiglu_bwd_c(d, last)
    ref, bnd = ec.swiglu_bwd_ref(c)
    assert ref["part"].shape[0] == 2 and (ref["part"][1] == 0).all()
    rc.check(ec.swiglu_bwd_f32(c, True)["part"], ref["part"], bnd["part"], "cpu rounds EPI5 part")
    Mq, _ = ec.rounds_shape(N_CU, ec.ROUNDS_QK_T)
    rows = gc.sample_rows(Mq)
    d = ec.qk_fused_case(Mq // ec.ROUNDS_QK_T, ec.ROUNDS_QK_T, 8, K, 2, 0, 43)
    c = ec.qk_fused_c(d, rows)
    ref, bnd = ec.qk_fused_ref(c, PRESCALE)
    got = ec.qk_fused_f32(c, PRESCALE)
    for k in got:
        rc.check(got[k], ref[k], bnd[k], f"cpu rounds EPI4 {k}")
