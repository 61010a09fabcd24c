"""The oracles of rowops_check.py have teeth (CPU only, no GPU): for every operation the fp32 restatements (autograd of
the plain forward at float32, and the one-pass formula at float32 with the column partials summed wave by wave) stay
inside the bounds at the shape classes of test_gpu_rowops.py, the bounds' own values equal the fp64 reference, and
seeded mutants - emulations of ways a kernel can go wrong - fall outside."""
import itertools
import math

import pytest
import torch

import rowops_check as rc

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


def fails(fn):
    with pytest.raises(AssertionError):
        fn()


def quiet(got, ref, bound):
    return lambda: rc.check_all(got, ref, bound, "mutant", verbose=False)


def default_nblk(M):
    return math.ceil(M / 4)


def inside(name, d, ev, formula, bounds, label, **kw):
    """reference, bounds (values = reference), and both fp32 restatements inside; returns (ref, bound, fp32 eval)"""
    ref = ev(d, **kw)
    vals, bnd = bounds(d, **kw)
    rc.close_values(vals, bnd, ref, label)
    got = ev(d, dtype=F32, **kw)
    rc.check_all(got, ref, bnd, f"cpu {name} autograd {label}")
    rc.check_all(formula(d, F32, **kw), ref, bnd, f"cpu {name} formula {label}")
    return ref, bnd, got


def waves_inside(rows32, key, ref, bnd, nblk, per_block, label):
    """the per-row terms summed as the kernel's waves sum them (+ the reduction) are inside the bound of the sum"""
    part = rc.wave_partials(rows32, nblk, per_block)
    assert part.shape[0] == (nblk if per_block else 4 * nblk)
    tot = rc.csr_eval(part, dtype=F32).reshape(ref[key].shape)
    rc.check(tot, ref[key], bnd[key], f"cpu {label} {key} by waves nblk={nblk}")


ROW_CLASSES = [(M, None) for M in rc.ROWS] + [rc.ONE_BLOCK]


# ------------------------------------------------------------------------------------------------ LERP
@pytest.mark.parametrize("C", rc.WIDTHS)
def test_lerp_fp32_inside_every_width(C):
    classes = ROW_CLASSES + ([rc.MULTI] if C in rc.MULTI_WIDTHS else [])
    for (M, nblk), skip in itertools.product(classes, (False, True)):
        d = rc.row_case(M, C, 10, skip=skip)
        label = f"lerp M{M} C{C} skip={skip}"
        ref, bnd, got = inside("lerp", d, rc.lerp_eval, rc.lerp_formula, rc.lerp_bounds, label)
        nb = nblk or default_nblk(M)
        waves_inside(got["dalpha_rows"], "dalpha", ref, bnd, nb, False, label)
        if skip:
            waves_inside(got["dskip_rows"], "dskip", ref, bnd, nb, False, label)


@pytest.mark.parametrize("C", rc.WIDTHS_SHORT + [260])
def test_lerp_option_product_inside(C):
    M, nblk = rc.MULTI
    for y_bf16, skip, add, accum in itertools.product((False, True), repeat=4):
        d = rc.row_case(M, C, 20, y_bf16=y_bf16, skip=skip, add=add, accum=accum)
        label = f"lerp C{C} ybf16={y_bf16} skip={skip} add={add} accum={accum}"
        ref, bnd, got = inside("lerp", d, rc.lerp_eval, rc.lerp_formula, rc.lerp_bounds, label)
        waves_inside(got["dalpha_rows"], "dalpha", ref, bnd, nblk, False, label)
        # a bf16 dy: one rounding to nearest even of the fp32 value stays inside the bound + half an ulp
        rc.check(got["dy"].bfloat16(), ref["dy"], bnd["dy"], f"cpu {label} dy_lo")


def test_lerp_forward_grid_stride_shape():
    for skip in (False, True):
        d = rc.row_case(rc.STRIDE_M, rc.STRIDE_C, 30, skip=skip)
        d["dout"] = None
        ref = rc.lerp_eval(d)
        vals, bnd = rc.lerp_bounds(d)
        rc.close_values(vals, bnd, ref, "lerp_fwd stride")
        rc.check_all(rc.lerp_eval(d, F32), ref, bnd, f"cpu lerp_fwd M{rc.STRIDE_M} skip={skip}")


# ------------------------------------------------------------------------------------------------ norm_skip, res_skip, rmsnorm
@pytest.mark.parametrize("C", rc.WIDTHS)
def test_norm_skip_and_res_skip_fp32_inside(C):
    classes = ROW_CLASSES + ([rc.MULTI] if C in rc.MULTI_WIDTHS else []) + ([(rc.STRIDE_M, None)] if C == 4 else [])
    for M, nblk in classes:
        Cc = rc.STRIDE_C if M == rc.STRIDE_M else C
        nb = nblk or min(1024, default_nblk(M))
        for tgt in (True, False):
            d = rc.row_case(M, Cc, 40)
            label = f"norm_skip M{M} C{Cc} tgt={tgt}"
            ref, bnd, got = inside("norm_skip", d, rc.norm_skip_eval, rc.norm_skip_formula, rc.norm_skip_bounds, label,
                                   tgt=tgt)
            waves_inside(got["dskip_rows"], "dskip", ref, bnd, nb, True, label)
        for y_bf16 in (False, True):
            d = rc.row_case(M, Cc, 50, y_bf16=y_bf16)
            label = f"res_skip M{M} C{Cc} ybf16={y_bf16}"
            ref, bnd, got = inside("res_skip", d, rc.res_skip_eval, rc.res_skip_formula, rc.res_skip_bounds, label)
            waves_inside(got["dskip_rows"], "dskip", ref, bnd, nb, False, label)
            rc.check(got["dh"].bfloat16(), ref["dh"], bnd["dh"], f"cpu {label} dh_lo")


@pytest.mark.parametrize("C", rc.WIDTHS)
def test_rmsnorm_and_res_rmsnorm_fp32_inside(C):
    classes = ROW_CLASSES + ([rc.MULTI] if C in rc.MULTI_WIDTHS else []) + ([(rc.STRIDE_M, None)] if C == 4 else [])
    for M, nblk in classes:
        Cc = rc.STRIDE_C if M == rc.STRIDE_M else C
        nb = nblk or min(1024, default_nblk(M))
        if Cc in rc.WIDTHS_SHORT + [rc.STRIDE_C]:
            d = rc.row_case(M, Cc, 60)
            label = f"rmsnorm M{M} C{Cc}"
            ref, bnd, got = inside("rmsnorm", d, rc.res_rmsnorm_eval, rc.res_rmsnorm_formula, rc.res_rmsnorm_bounds,
                                   label, with_y=False)
            waves_inside(got["dw_rows"], "dw", ref, bnd, nb, True, label)
        opts = itertools.product((None, F32, BF16), (False, True), (False, True)) if Cc in rc.WIDTHS_SHORT else \
            [(F32, False, False), (None, False, False)]
        for ydt, add, accum in opts:
            d = rc.row_case(M, Cc, 70, y_bf16=ydt == BF16, add=add, accum=accum)
            label = f"res_rmsnorm M{M} C{Cc} y={ydt} add={add} accum={accum}"
            ref, bnd, got = inside("res_rmsnorm", d, rc.res_rmsnorm_eval, rc.res_rmsnorm_formula,
                                   rc.res_rmsnorm_bounds, label, with_y=ydt is not None)
            waves_inside(got["dw_rows"], "dw", ref, bnd, nb, False, label)


# ------------------------------------------------------------------------------------------------ q/k normalise
def qk_given(c, dt):
    """the tensors a backward kernel is handed in mode dt: the fp32 forward, the head tensors rounded to dt"""
    f = rc.qknorm_eval(c, F32)
    return {"qh": f["qh"].to(dt), "kh": f["kh"].to(dt), "rq": f["rq"], "rk": f["rk"]}


@pytest.mark.parametrize("H,d", rc.QK_HEADS)
def test_qknorm_fp32_inside(H, d):
    for (B, T), in_dt in itertools.product((rc.QK_BT, (1, rc.ONE_BLOCK[0])), (F32, BF16)):
        c = rc.qk_case(B, T, H, d, 80, in_dt)
        label = f"qknorm B{B} T{T} H{H} d{d} in={in_dt}"
        ref = rc.qknorm_eval(c)
        vals, bnd = rc.qknorm_bounds(c)
        rc.close_values(vals, bnd, ref, label)
        got = rc.qknorm_eval(c, F32)
        rc.check_all(got, ref, bnd, f"cpu {label} autograd")
        fwd32 = rc.qknorm_fwd_formula(c, F32)
        rc.check_all(fwd32, ref, {k: bnd[k] for k in fwd32}, f"cpu {label} formula fwd")
        bwd_keys = ("dq", "dk", "dsqk")
        rc.check_all(rc.qknorm_bwd_formula(c, fwd32, F32), ref, {k: bnd[k] for k in bwd_keys},
                     f"cpu {label} formula bwd")
        rc.check_all({k: got[k].bfloat16() for k in ("qh", "kh", "dq", "dk")}, ref,
                     {k: bnd[k] for k in ("qh", "kh", "dq", "dk")}, f"cpu {label} bf16 outputs")
        nb = rc.ONE_BLOCK[1] if T == rc.ONE_BLOCK[0] else 3 if (H, d) == rc.QK_MULTI else default_nblk(B * T)
        waves_inside(got["dsqk_rows"], "dsqk", ref, bnd, nb, True, label)
        for dt in (F32, BF16):      # the second reference: the formula in fp64 on the tensors handed over
            given = qk_given(c, dt)
            ref2 = rc.qknorm_bwd_formula(c, given, F64)
            vals2, bnd2 = rc.qknorm_bounds(c, given)
            rc.close_values(vals2, bnd2, ref2, label)
            rc.check_all(rc.qknorm_bwd_formula(c, given, F32), ref2, bnd2, f"cpu {label} given {dt}")


def test_qknorm_forward_grid_stride_shape():
    c = rc.qk_case(*rc.QK_STRIDE, 85)
    ref = rc.qknorm_eval(c)
    fwd32 = rc.qknorm_fwd_formula(c, F32)
    _, bnd = rc.qknorm_bounds(c)
    rc.check_all(fwd32, ref, {k: bnd[k] for k in fwd32}, "cpu qknorm_fwd stride")


# ------------------------------------------------------------------------------------------------ SwiGLU
@pytest.mark.parametrize("F", rc.SWIGLU_F)
def test_swiglu_fp32_inside(F):
    for M in rc.SWIGLU_M + ([rc.SWIGLU_TALL[0]] if F == rc.SWIGLU_TALL[1] else []):
        for use_suv, dt in itertools.product((False, True), (F32, BF16)):
            c = rc.swiglu_case(M, F, 90, use_suv, dt)
            label = f"swiglu M{M} F{F} suv={use_suv} {dt}"
            ref = rc.swiglu_eval(c)
            vals, bnd = rc.swiglu_bounds(c)
            rc.close_values(vals, bnd, ref, label)
            got = rc.swiglu_eval(c, F32)
            rc.check_all(got, ref, bnd, f"cpu {label} autograd")
            rc.check_all(rc.swiglu_formula(c, F32), ref, bnd, f"cpu {label} formula")
            rc.check_all({k: got[k].bfloat16() for k in ("x", "duv")}, ref, {k: bnd[k] for k in ("x", "duv")},
                         f"cpu {label} bf16 outputs")
            if use_suv:
                fails(quiet(rc.swiglu_eval(c, F32, dv_mutant=True), ref, bnd))   # dv without v * (1 - sg)
    assert torch.equal(rc.deinterleave(rc.interleave(c["uv"], F), F), c["uv"])


# ------------------------------------------------------------------------------------------------ colsum_reduce
def csr_cases():
    for nblk, N in itertools.product(rc.CSR_NBLK, rc.CSR_N):
        for kind in (0, 1):
            yield nblk, N, kind
    for nblk, N in itertools.product(rc.CSR_NBLK, rc.CSR_N_KIND2):
        yield nblk, N, 2


def test_colsum_reduce_exact_on_integers_bounded_on_gauss_and_mutants_fail():
    for nblk, N, kind in csr_cases():
        for accumulate, nblk_b in itertools.product((False, True), (0, 5)):
            c = rc.csr_int_case(nblk, N, 100, kind, accumulate, nblk_b)
            ref = rc.csr_ref(c)
            rc.assert_exact(rc.csr_ref(c, F32), ref, f"csr int nblk{nblk} N{N} kind{kind}")
            g = rc.csr_gauss_case(nblk, N, 101, kind, accumulate, nblk_b)
            rc.check(rc.csr_ref(g, F32), rc.csr_ref(g), rc.csr_case_bound(g),
                     f"cpu csr nblk{nblk} N{N} kind{kind} acc={accumulate} b={nblk_b}",
                     verbose=nblk in (33, 4096) and N == 260)
            # (at N = 32 the kind-2 destination is the identity: one block of 16 u and 16 v is already u | v)
            muts = (["sign"] if kind == 1 else []) + (["dst"] if kind == 2 and N > 32 else []) + \
                   (["accumulate"] if accumulate else []) + (["part_b"] if nblk_b else [])
            for m in muts:
                bad = rc.csr_ref(c, F32, m)
                if not torch.equal(bad, ref.float()):       # (integer sums can cancel; the Gaussian ones do not)
                    fails(lambda: rc.assert_exact(bad, ref, "mutant"))
                fails(lambda: rc.check(rc.csr_ref(g, F32, m), rc.csr_ref(g), rc.csr_case_bound(g), "mutant",
                                       verbose=False))
            if nblk > 1:    # a dropped, a doubled and a misplaced partial row
                p = c["part"]
                for bad_part in (p[:-1], torch.cat([p, p[nblk // 2:nblk // 2 + 1]]), ):
                    bad = rc.csr_ref(dict(c, part=bad_part), F32)
                    if p[-1].abs().sum() > 0 and p[nblk // 2].abs().sum() > 0 and N > 1:
                        fails(lambda: rc.assert_exact(bad, ref, "mutant"))


def test_kind1_sign_needs_a_negative_alpha():
    c = rc.csr_int_case(33, 32, 102, 1, False)
    assert (c["ref"] < 0).any() and (c["ref"] > 0).any() and (c["ref"] != 0).all()
    d = rc.row_case(3, 4, 1)
    assert (d["alpha"] < 0).any() and (d["alpha"] > 0).any()


# ------------------------------------------------------------------------------------------------ mutants of 
def lerp_mutant_setup(M, C, nblk, **opt):
    d = rc.row_case(M, C, 110, **opt)
    ref = rc.lerp_eval(d)
    _, bnd = rc.lerp_bounds(d)
    return d, ref, bnd, rc.lerp_eval(d, F32)


def test_mutant_column_sum_keeps_last_row_of_each_wave():
    """3 rows per wave: M = 12 on one workgroup; both partial layouts and the scalar sums"""
    M, nblk, C = 12, 1, 4
    assert all(len(v) == 3 for v in rc.wave_visits(M, nblk))
    d, ref, bnd, got = lerp_mutant_setup(M, C, nblk, skip=True)
    for key, rows in (("dalpha", got["dalpha_rows"]), ("dskip", got["dskip_rows"])):
        waves_inside(rows, key, ref, bnd, nblk, False, "lerp")
        bad = rc.csr_eval(rc.wave_partials(rows, nblk, keep_last=True), dtype=F32).reshape(ref[key].shape)
        fails(lambda: rc.check(bad, ref[key], bnd[key], "mutant", verbose=False))
    ref = rc.res_rmsnorm_eval(d, with_y=False)
    _, bnd = rc.res_rmsnorm_bounds(d, with_y=False)
    rows = rc.res_rmsnorm_eval(d, F32, with_y=False)["dw_rows"]
    bad = rc.csr_eval(rc.wave_partials(rows, nblk, True, keep_last=True), dtype=F32)
    fails(lambda: rc.check(bad, ref["dw"], bnd["dw"], "mutant", verbose=False))
    c = rc.qk_case(1, M, 1, 16, 111)
    ref = rc.qknorm_eval(c)
    _, bnd = rc.qknorm_bounds(c)
    rows = rc.qknorm_eval(c, F32)["dsqk_rows"]
    waves_inside(rows, "dsqk", ref, bnd, nblk, True, "qknorm")
    bad = rc.csr_eval(rc.wave_partials(rows, nblk, True, keep_last=True), dtype=F32)
    fails(lambda: rc.check(bad, ref["dsqk"], bnd["dsqk"], "mutant", verbose=False))


def test_mutant_row_stride_off_by_one_wave():
    """the last wave's stride is one row short: a row of its neighbour is counted twice, its own second row never"""
    M, nblk, C = 9, 1, 4
    visits = rc.wave_visits(M, nblk)
    assert visits[3] == [3, 7]
    visits[3] = [3, 6]
    flat = sorted(m for v in visits for m in v)
    assert flat.count(6) == 2 and 7 not in flat
    d, ref, bnd, got = lerp_mutant_setup(M, C, nblk, skip=True)
    for key, rows in (("dalpha", got["dalpha_rows"]), ("dskip", got["dskip_rows"])):
        bad = rc.csr_eval(rc.wave_partials(rows, nblk, visits=visits), dtype=F32).reshape(ref[key].shape)
        fails(lambda: rc.check(bad, ref[key], bnd[key], "mutant", verbose=False))
    # the element-wise outputs: row 7 holds what row 6 got
    bad = dict(got)
    bad["dh"] = got["dh"].clone()
    bad["dh"][7] = got["dh"][6]
    fails(quiet(bad, ref, bnd))


@pytest.mark.parametrize("C", [260, 1028])
def test_mutant_last_float4_group_left_out_of_the_row_norm(C, monkeypatch):
    d = rc.row_case(3, C, 120, skip=True)
    refs = [(rc.lerp_eval, rc.lerp_bounds, {}), (rc.norm_skip_eval, rc.norm_skip_bounds, {}),
            (rc.res_skip_eval, rc.res_skip_bounds, {})]
    computed = [(ev, ev(d), bounds(d)[1]) for ev, bounds, _ in refs]
    monkeypatch.setattr(rc.O, "nrm", lambda x: x / torch.sqrt((x[..., :-4] * x[..., :-4]).sum(dim=-1, keepdim=True)))
    for ev, ref, bnd in computed:
        bad = ev(d, F32)
        fails(lambda: rc.check(bad["out"], ref["out"], bnd["out"], "mutant", verbose=False))
        fails(quiet(bad, ref, bnd))
    # RMSNorm: the mean of squares without the last four columns
    ref = rc.res_rmsnorm_eval(d, with_y=False)
    _, bnd = rc.res_rmsnorm_bounds(d, with_y=False)
    x = d["h"]
    bad = x * torch.rsqrt((x[:, :-4] ** 2).sum(-1, keepdim=True) / C + d["eps"]) * d["w"]
    fails(lambda: rc.check(bad, ref["out"], bnd["out"], "mutant", verbose=False))


@pytest.mark.parametrize("H,d,group", [(3, 16, 32), (2, 32, 64), (5, 128, 64)])
def test_mutant_head_norm_over_two_heads_or_half_a_head(H, d, group):
    c = rc.qk_case(*rc.QK_BT, H, d, 130)
    ref = rc.qknorm_eval(c)
    _, bnd = rc.qknorm_bounds(c)
    bad = rc.qknorm_eval(c, F32, group=group)
    for k in ("qh", "kh", "dq", "dk", "dsqk"):
        fails(lambda: rc.check(bad[k], ref[k], bnd[k], "mutant", verbose=False))


def test_mutant_out_lo_truncated_instead_of_rounded():
    d = rc.row_case(3, 260, 140)
    out = rc.lerp_eval(d, F32)["out"]
    rc.rounded_copy(out.bfloat16(), out, "out_lo")
    trunc = (out.view(torch.int32) & -65536).view(F32).bfloat16()
    assert not torch.equal(trunc, out.bfloat16())
    fails(lambda: rc.rounded_copy(trunc, out, "mutant"))


def test_mutant_accumulate_or_addend_ignored():
    M, C = 5, 260
    for ev, bounds, key in ((rc.lerp_eval, rc.lerp_bounds, "dh"), (rc.res_rmsnorm_eval, rc.res_rmsnorm_bounds, "dz")):
        d = rc.row_case(M, C, 150, add=True, accum=True)
        ref = ev(d)
        _, bnd = bounds(d)
        rc.check_all(ev(d, F32), ref, bnd, f"cpu {key} add + accumulate")
        fails(quiet(ev(dict(d, old=None), F32), ref, bnd))          # accumulate ignored
        fails(quiet(ev(dict(d, dout_add=None), F32), ref, bnd))     # the addend of the incoming gradient ignored
