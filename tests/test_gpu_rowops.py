"""GPU tests, op level: the row kernels of rowops.hip (LERP, norm_skip, RMSNorm, residual + RMSNorm, residual +
norm_skip, q/k normalise, the SwiGLU gate, the column-partial reductions) through nvit_amd.ops against the fp64
references and per-element bounds of rowops_check.py: every width class of the 1, 2, 3, 4 and 8-vector instantiations,
waves that walk no row, one row and several rows (the `nblk` override of the backward wrappers), the forward grid
stride, every element type and row stride.  test_rowops_check.py shows on the CPU that these bounds pass a correct fp32
restatement and fail the mutants named there.  Run on the MI355X box: pytest -m gpu."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

import kohonen_check as kc
import rowops_check as rc

F32T, F64T, BF16T = torch.float32, torch.float64, torch.bfloat16
NAN = float("nan")


def dev():
    return torch.device("cuda:0")


def ops_():
    from nvit_amd import ops
    return ops


def modes():
    from nvit_amd import _lib
    return _lib.F32, _lib.BF16, _lib.BF16_F32IN


def D(t):
    return None if t is None else t.to(dev())


def poison(*shape, dtype=F32T):
    return torch.full(shape, NAN, device=dev(), dtype=dtype)


def td(dt):
    return F32T if dt == modes()[0] else BF16T


def row_classes(C):
    """(M, nblk): default grids with idle waves, one workgroup with 2-3 rows per wave, 12 waves with 3-4 rows"""
    return [(M, None) for M in rc.ROWS] + [rc.ONE_BLOCK] + ([rc.MULTI] if C in rc.MULTI_WIDTHS else [])


def idle_waves_wrote_zeros(part, M, label):
    """wave g walks rows g, g + waves, ...: a wave past the last row must still store its (zero) partials"""
    idle = part[M:]
    assert torch.equal(idle, torch.zeros_like(idle)), f"{label}: partials of waves without a row are not zero"


def reduce_(part, n, **kw):
    out = poison(n)
    ops_().colsum_reduce(part, out, False, **kw)
    return out


# ------------------------------------------------------------------------------------------------ LERP
def run_lerp(d, dt, nblk, want_dy, label):
    ops = ops_()
    M, C = d["h"].shape
    h, y, alpha, xs, skip = D(d["h"]), D(d["y"]), D(d["alpha"]), D(d["skip_x"]), D(d["skip"])
    out, out_lo = ops.lerp_fwd(dt, h, y, alpha, d["c_a"], skip_x=xs, skip=skip, want_lo=True)
    rc.rounded_copy(out_lo, out, label + " out_lo")
    accum = d["old"] is not None
    dh0 = D(d["old"]).clone() if accum else poison(M, C)
    dh, dy, dy_lo, dxs, part, pskip = ops.lerp_bwd(dt, D(d["dout"]), h, y, alpha, d["c_a"], xs, skip, dh0, accum, want_dy,
                                                   True, dout_add=D(d["dout_add"]), nblk=nblk)
    assert dh.data_ptr() == dh0.data_ptr() and dy_lo.dtype == td(dt) and (dy is None) == (not want_dy)
    if nblk is not None:
        assert tuple(part.shape) == (4 * nblk, C)
    idle_waves_wrote_zeros(part, M, label)
    got = {"out": out, "dh": dh, "dy": dy if want_dy else dy_lo,
           "dalpha": reduce_(part, C, kind=1, ref=alpha, scale=d["c_a"])}
    if want_dy:
        rc.rounded_copy(dy_lo, dy, label + " dy_lo")
    if xs is not None:
        assert tuple(pskip.shape) == (part.shape[0],)
        idle_waves_wrote_zeros(pskip, M, label)
        got.update(dskip_x=dxs, dskip=reduce_(pskip, 1))
    else:
        assert dxs is None and pskip is None
    _, bnd = rc.lerp_bounds(d)
    return rc.check_all(got, rc.lerp_eval(d), bnd, label)


@pytest.mark.parametrize("C", rc.WIDTHS)
def test_lerp_fwd_bwd_every_width(C):
    F32 = modes()[0]
    for (M, nblk), skip in itertools.product(row_classes(C), (False, True)):
        run_lerp(rc.row_case(M, C, 10, skip=skip), F32, nblk, True, f"lerp M{M} C{C} nblk={nblk} skip={skip}")


@pytest.mark.parametrize("C", rc.WIDTHS_SHORT + [260])
def test_lerp_bwd_option_product(C):
    """y fp32 / bf16 x dt fp32 / bf16 x skip x dout_add x accumulate; a multi-row wave in every option at 260, 1028"""
    F32, BF16, _ = modes()
    M, nblk = rc.MULTI if C in rc.MULTI_WIDTHS else (rc.MULTI[0], None)
    for dt, y_bf16, skip, add, accum in itertools.product((F32, BF16), *[(False, True)] * 4):
        d = rc.row_case(M, C, 20, y_bf16=y_bf16, skip=skip, add=add, accum=accum)
        run_lerp(d, dt, nblk, not add, f"lerp C{C} nblk={nblk} dt={dt} ybf16={y_bf16} skip={skip} add={add} acc={accum}")


# ------------------------------------------------------------------------------------------------ norm_skip
@pytest.mark.parametrize("C", rc.WIDTHS)
def test_norm_skip_fwd_bwd_every_width(C):
    ops = ops_()
    for (M, nblk), tgt in itertools.product(row_classes(C), (True, False)):
        d = rc.row_case(M, C, 40)
        label = f"norm_skip M{M} C{C} nblk={nblk} tgt={tgt}"
        src, x, skip = D(d["h"]), D(d["x"]) if tgt else None, D(d["skip1"])
        out = ops.norm_skip_fwd(src, x, skip)
        dsrc, dtgt, dskip = ops.norm_skip_bwd(D(d["dout"]), src, x, skip, nblk=nblk)
        got = {"out": out, "dsrc": dsrc, "dskip": dskip}
        if tgt:
            got["dtgt"] = dtgt
        else:
            assert dtgt is None
        _, bnd = rc.norm_skip_bounds(d, tgt=tgt)
        rc.check_all(got, rc.norm_skip_eval(d, tgt=tgt), bnd, label)


# ------------------------------------------------------------------------------------------------ residual + norm_skip
@pytest.mark.parametrize("C", rc.WIDTHS)
def test_res_skip_fwd_bwd_every_width(C):
    ops = ops_()
    F32, BF16, _ = modes()
    types = list(itertools.product((F32, BF16), (False, True))) if C in rc.WIDTHS_SHORT else [(F32, False)]
    for (M, nblk), (dt, y_bf16) in itertools.product(row_classes(C), types):
        d = rc.row_case(M, C, 50, y_bf16=y_bf16)
        label = f"res_skip M{M} C{C} nblk={nblk} dt={dt} ybf16={y_bf16}"
        h, y, skip, x = D(d["h"]), D(d["y"]), D(d["skip1"]), D(d["x"])
        out, out_lo = ops.res_skip_fwd(dt, h, y, skip, x, want_lo=True)
        rc.rounded_copy(out_lo, out, label + " out_lo")
        dh, dh_lo, dx, part = ops.res_skip_bwd(dt, D(d["dout"]), h, y, skip, x, want_lo=True, nblk=nblk)
        assert dh_lo.dtype == td(dt)
        rc.rounded_copy(dh_lo, dh, label + " dh_lo")
        if nblk is not None:
            assert tuple(part.shape) == (4 * nblk,)
        idle_waves_wrote_zeros(part, M, label)
        _, bnd = rc.res_skip_bounds(d)
        rc.check_all({"out": out, "dh": dh, "dx": dx, "dskip": reduce_(part, 1)}, rc.res_skip_eval(d), bnd, label)


# ------------------------------------------------------------------------------------------------ RMSNorm
@pytest.mark.parametrize("C", rc.WIDTHS_SHORT)
def test_rmsnorm_fwd_bwd(C):
    ops = ops_()
    for M, nblk in row_classes(C):
        d = rc.row_case(M, C, 60)
        label = f"rmsnorm M{M} C{C} nblk={nblk}"
        x, w = D(d["h"]), D(d["w"])
        out, rstd = ops.rmsnorm_fwd(x, w, d["eps"])
        dx, dw = ops.rmsnorm_bwd(D(d["dout"]), x, w, rstd, nblk=nblk)
        _, bnd = rc.res_rmsnorm_bounds(d, with_y=False)
        rc.check_all({"out": out, "rstd": rstd, "dz": dx, "dw": dw}, rc.res_rmsnorm_eval(d, with_y=False), bnd, label)


@pytest.mark.parametrize("C", rc.WIDTHS)
def test_res_rmsnorm_fwd_bwd_every_width(C):
    """y None / fp32 / bf16 x dt x g_add x accumulate at the short list of widths, the plain call at every width"""
    ops = ops_()
    F32, BF16, _ = modes()
    if C in rc.WIDTHS_SHORT:
        opts = list(itertools.product((F32, BF16), (None, F32T, BF16T), (False, True), (False, True)))
    else:
        opts = [(F32, F32T, False, False), (F32, None, False, False)]
    for (M, nblk), (dt, ydt, add, accum) in itertools.product(row_classes(C), opts):
        d = rc.row_case(M, C, 70, y_bf16=ydt == BF16T, add=add, accum=accum, g_add_dtype=td(dt))
        label = f"res_rmsnorm M{M} C{C} nblk={nblk} dt={dt} y={ydt} add={add} acc={accum}"
        a, y, w = D(d["h"]), D(d["y"]) if ydt is not None else None, D(d["w"])
        out, out_lo, rstd = ops.res_rmsnorm_fwd(dt, a, y, w, d["eps"], want_lo=True)
        rc.rounded_copy(out_lo, out, label + " out_lo")
        dz0 = D(d["old"]).clone() if accum else None
        dz, dz_lo, part = ops.res_rmsnorm_bwd(dt, D(d["dout"]), a, y, w, rstd, g_add=D(d["dout_add"]), dz=dz0,
                                              want_lo=True, nblk=nblk)
        assert not accum or dz.data_ptr() == dz0.data_ptr()
        rc.rounded_copy(dz_lo, dz, label + " dz_lo")
        if nblk is not None:
            assert tuple(part.shape) == (4 * nblk, C)
        idle_waves_wrote_zeros(part, M, label)
        _, bnd = rc.res_rmsnorm_bounds(d, with_y=ydt is not None)
        rc.check_all({"out": out, "rstd": rstd, "dz": dz, "dw": reduce_(part, C)},
                     rc.res_rmsnorm_eval(d, with_y=ydt is not None), bnd, label)


# ------------------------------------------------------------------------------------------------ forward grid stride
def test_forward_kernels_grid_stride():
    """8197 rows: the 2048-workgroup forward grids walk 8192 rows per sweep, five rows are left for a second one"""
    ops = ops_()
    F32 = modes()[0]
    M, C = rc.STRIDE_M, rc.STRIDE_C
    d = rc.row_case(M, C, 30, skip=True)
    d["dout"] = None
    h, y, alpha, xs, skip, w = (D(d[k]) for k in ("h", "y", "alpha", "skip_x", "skip", "w"))
    for with_skip in (False, True):
        dd = d if with_skip else dict(d, skip_x=None, skip=None)
        out, out_lo = ops.lerp_fwd(F32, h, y, alpha, d["c_a"], skip_x=xs if with_skip else None,
                                   skip=skip if with_skip else None)
        rc.rounded_copy(out_lo, out, "lerp_fwd stride out_lo")
        rc.check(out, rc.lerp_eval(dd)["out"], rc.lerp_bounds(dd)[1]["out"], f"lerp_fwd M{M} skip={with_skip}")
    d["dout"] = rc.gauss_data((M, C), 31)      # (the references below compute a backward as well)
    for tgt in (True, False):
        out = ops.norm_skip_fwd(h, xs if tgt else None, skip)
        rc.check(out, rc.norm_skip_eval(d, tgt=tgt)["out"], rc.norm_skip_bounds(d, tgt=tgt)[1]["out"],
                 f"norm_skip_fwd M{M} tgt={tgt}")
    out, rstd = ops.rmsnorm_fwd(h, w, d["eps"])
    ref, bnd = rc.res_rmsnorm_eval(d, with_y=False), rc.res_rmsnorm_bounds(d, with_y=False)[1]
    rc.check_all({"out": out, "rstd": rstd}, ref, {k: bnd[k] for k in ("out", "rstd")}, f"rmsnorm_fwd M{M}")
    for with_y in (False, True):
        out, _, rstd = ops.res_rmsnorm_fwd(F32, h, y if with_y else None, w, d["eps"])
        ref, bnd = rc.res_rmsnorm_eval(d, with_y=with_y), rc.res_rmsnorm_bounds(d, with_y=with_y)[1]
        rc.check_all({"out": out, "rstd": rstd}, ref, {k: bnd[k] for k in ("out", "rstd")},
                     f"res_rmsnorm_fwd M{M} y={with_y}")
    out, _ = ops.res_skip_fwd(F32, h, y, skip, xs)
    rc.check(out, rc.res_skip_eval(d)["out"], rc.res_skip_bounds(d)[1]["out"], f"res_skip_fwd M{M}")
    c = rc.qk_case(*rc.QK_STRIDE, 85)
    B, T, H, dh = rc.QK_STRIDE
    qkv = D(torch.cat([c["q"], c["k"], c["v"]], dim=1))
    Cq = H * dh
    qh, kh, vh, rq, rk = ops.qknorm_fwd(F32, qkv, 3 * Cq, qkv[:, Cq:], 3 * Cq, qkv[:, 2 * Cq:], 3 * Cq, D(c["sqk"]),
                                        c["c_q"], B, T, H, dh)
    ref, bnd = rc.qknorm_eval(c), rc.qknorm_bounds(c)[1]
    rc.check_all({"qh": qh, "kh": kh, "rq": rq, "rk": rk}, ref, {k: bnd[k] for k in ("qh", "kh", "rq", "rk")},
                 f"qknorm_fwd T{T}")
    assert rc.bits_equal(vh.cpu(), ref["vh"].float().contiguous())


# ------------------------------------------------------------------------------------------------ q/k normalise
def qk_buffers(mats, layout, C, dtype, fill=None):
    """three [M, C] operands in one fused [M, 3C] buffer (ld = 3C), or in separate buffers with ld = C or ld = C + 8
    whose padding columns hold the sentinel.  mats None: output buffers, poisoned.  -> (views, ld, buffers)"""
    M = mats[0].shape[0] if mats is not None else fill
    if layout == "fused":
        buf = poison(M, 3 * C, dtype=dtype)
        if mats is not None:
            buf.copy_(torch.cat(mats, dim=1))
        return [buf[:, i * C:] for i in range(3)], 3 * C, [buf]
    ld = C if layout == "sep" else C + 8
    bufs = []
    for i in range(3):
        b = torch.full((M, ld), rc.SENTINEL, device=dev(), dtype=dtype)
        b[:, :C] = NAN if mats is None else D(mats[i]).to(dtype)
        bufs.append(b)
    return bufs, ld, bufs


def run_qknorm(c, mode, layout, nblk, label):
    """mode: the forward's dt.  F32: fp32 in and out, backward in F32 against both references; BF16: bf16 in and out;
    BF16_F32IN: fp32 in, bf16 head tensors; the backward of both runs in BF16 from the forward's own outputs."""
    ops = ops_()
    F32, BF16, BF16_F32IN = modes()
    B, T, H, d = c["B"], c["T"], c["H"], c["d"]
    M, C = B * T, H * d
    in_dt = BF16T if mode == BF16 else F32T
    out_dt = F32T if mode == F32 else BF16T
    c = dict(c, **{n: c[n].to(in_dt) for n in ("q", "k", "v")})
    c.update({n: c[n].to(out_dt) for n in ("gq", "gk", "gv")})       # the incoming gradients are exact inputs too
    (q, k, v), ld, _ = qk_buffers([c["q"], c["k"], c["v"]], layout, C, in_dt)
    sqk = D(c["sqk"])
    qh, kh, vh, rq, rk = ops.qknorm_fwd(mode, q, ld, k, ld, v, ld, sqk, c["c_q"], B, T, H, d)
    assert qh.dtype == out_dt and tuple(qh.shape) == (B, H, T, d)
    ref = rc.qknorm_eval(c)
    _, bnd = rc.qknorm_bounds(c)
    fwd_keys = ("qh", "kh", "rq", "rk")
    rc.check_all({"qh": qh, "kh": kh, "rq": rq, "rk": rk}, ref, {n: bnd[n] for n in fwd_keys}, label + " fwd")
    assert rc.bits_equal(vh.cpu(), ref["vh"].to(out_dt).contiguous()), f"{label}: vh is not a copy of v"
    bdt = F32 if mode == F32 else BF16
    (dq, dk, dv), ldo, bufs = qk_buffers(None, layout, C, out_dt, fill=M)
    part = ops.qknorm_bwd(bdt, D(c["gq"]), D(c["gk"]), D(c["gv"]), qh, kh, rq, rk, sqk, c["c_q"], dq, ldo, dk, ldo, dv,
                          ldo, B, T, H, d, nblk=nblk)
    if nblk is not None:
        assert tuple(part.shape) == (nblk, C)
    for b in bufs:
        if layout == "pad":
            assert (b[:, C:] == rc.SENTINEL).all(), f"{label}: the padding columns were written"
    got = {"dq": dq[:, :C], "dk": dk[:, :C], "dsqk": reduce_(part, C, kind=0, scale=c["c_q"])}
    given = {"qh": qh.cpu(), "kh": kh.cpu(), "rq": rq.cpu(), "rk": rk.cpu()}
    vals2, bnd2 = rc.qknorm_bounds(c, given)
    rc.check_all(got, rc.qknorm_bwd_formula(c, given, F64T), bnd2, label + " bwd (formula on the kernel's tensors)")
    if mode == F32:
        rc.check_all(got, ref, {n: bnd[n] for n in got}, label + " bwd (autograd)")
    assert rc.bits_equal(dv[:, :C].cpu().contiguous(), rc.from_heads(c["gv"], B, T, H, d).contiguous()), \
        f"{label}: dv is not a copy of dvh"


@pytest.mark.parametrize("H,d", rc.QK_HEADS)
def test_qknorm_fwd_bwd_heads_types_strides(H, d):
    B, T = rc.QK_BT
    c = rc.qk_case(B, T, H, d, 80)
    for mode, layout in itertools.product(modes(), ("fused", "sep", "pad")):
        run_qknorm(c, mode, layout, None, f"qknorm H{H} d{d} mode={mode} {layout}")
    for mode in modes():
        if (H, d) == rc.QK_MULTI:
            run_qknorm(c, mode, "fused", 3, f"qknorm H{H} d{d} mode={mode} nblk=3")
        M1, nb1 = rc.ONE_BLOCK
        run_qknorm(rc.qk_case(1, M1, H, d, 81), mode, "pad", nb1, f"qknorm H{H} d{d} T{M1} mode={mode} nblk={nb1}")


# ------------------------------------------------------------------------------------------------ SwiGLU
@pytest.mark.parametrize("F", rc.SWIGLU_F)
def test_swiglu_fwd_bwd(F):
    """interleaved (16 u | 16 v) layout in and out; the d(suv) partials reduced as the block's backward reduces them
    (kind 0, scale 1), the interleaved duv column sums as the fc bias gradient takes them (colsum modulo 512, kind 2)."""
    ops = ops_()
    F32, BF16, BF16_F32IN = modes()
    for M in rc.SWIGLU_M + ([rc.SWIGLU_TALL[0]] if F == rc.SWIGLU_TALL[1] else []):
        for use_suv, mode in itertools.product((False, True), (F32, BF16, BF16_F32IN)):
            in_dt = BF16T if mode == BF16 else F32T
            out_dt = F32T if mode == F32 else BF16T
            c = rc.swiglu_case(M, F, 90, use_suv, in_dt)
            label = f"swiglu M{M} F{F} suv={use_suv} mode={mode}"
            uvi, suv = D(rc.interleave(c["uv"], F).contiguous()), D(c["suv"])
            x = ops.swiglu_fwd(mode, uvi, suv, c["gscale"], M, F)
            assert x.dtype == out_dt
            ref = rc.swiglu_eval(c)
            _, bnd = rc.swiglu_bounds(c)
            rc.check(x, ref["x"], bnd["x"], label + " x")
            if mode == BF16_F32IN:
                continue                    # (the backward has no mixed mode)
            duv, part = ops.swiglu_bwd(mode, D(c["dx"]), uvi, suv, c["gscale"], M, F)
            got = {"duv": rc.deinterleave(duv.cpu(), F)}
            if use_suv:
                got["dsuv"] = reduce_(part, 2 * F, kind=0, scale=1.0)
            else:
                assert part is None
            rc.check_all(got, ref, {n: bnd[n] for n in got}, label)
            # column sums of the interleaved duv in natural order (the bias gradient of fc)
            p512 = poison(512, 2 * F)
            ops.colsum(duv, M, 2 * F, p512, False, period=512)
            g = poison(2 * F)
            ops.colsum_reduce(p512, g, False, kind=2)
            want, bound = kc.colsum_ref(got["duv"], None, M, 2 * F, 1, 1.0)      # of the duv the kernel wrote
            rc.check(g, want.reshape(-1), bound.reshape(-1), label + " colsum kind 2")


# ------------------------------------------------------------------------------------------------ colsum_reduce
def run_csr(c, label, exact, batch=None):
    """one reduction through ops.colsum_reduce (or queued on `batch`); the output sits in a longer buffer whose tail
    holds the sentinel.  Returns the closure that checks it (after the flush)."""
    N = c["part"].shape[1] if c["part"].dim() == 2 else 1
    buf = torch.full((N + 8,), rc.SENTINEL, device=dev())
    buf[:N] = D(c["old"]) if c["old"] is not None else NAN
    out = buf[:N]
    args = dict(kind=c["kind"], ref=D(c["ref"]), scale=c["scale"])
    if batch is None:
        assert c["part_b"] is None
        ops_().colsum_reduce(D(c["part"]), out, c["old"] is not None, **args)
    else:
        batch.add(D(c["part"]), out, c["old"] is not None, part_b=D(c["part_b"]), **args)

    def verify():
        assert (buf[N:] == rc.SENTINEL).all(), f"{label}: wrote past N"
        if exact:
            assert torch.isfinite(out).all(), f"{label}: unwritten output"
            rc.assert_exact(out.cpu(), rc.csr_ref(c), label)
        else:
            rc.check(out, rc.csr_ref(c), rc.csr_case_bound(c), label)
    return verify


def csr_widths(kind):
    return rc.CSR_N_KIND2 if kind == 2 else rc.CSR_N


@pytest.mark.parametrize("nblk", rc.CSR_NBLK)
def test_colsum_reduce_exact_every_edge(nblk):
    """integer partials and a power-of-two scale: bit-identical to the fp64 sum whatever the order"""
    for kind in (0, 1, 2):
        for N, accumulate in itertools.product(csr_widths(kind), (False, True)):
            label = f"colsum_reduce nblk{nblk} N{N} kind{kind} acc={accumulate}"
            run_csr(rc.csr_int_case(nblk, N, 100, kind, accumulate), label, True)()
            batch = ops_().ReduceBatch()            # the multi kernel: a second partial array of another row count
            v = run_csr(rc.csr_int_case(nblk, N, 103, kind, accumulate, nblk_b=max(1, nblk // 2 + 1)),
                        label + " part_b", True, batch)
            batch.flush()
            v()


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_colsum_reduce_gauss_against_bound(kind):
    N = csr_widths(kind)[-1]
    for nblk, accumulate in itertools.product((129, 4096), (False, True)):
        run_csr(rc.csr_gauss_case(nblk, N, 101, kind, accumulate), f"colsum_reduce gauss nblk{nblk} N{N} kind{kind}", False)()
        batch = ops_().ReduceBatch()
        v = run_csr(rc.csr_gauss_case(nblk, N, 104, kind, accumulate, nblk_b=33), f"multi gauss nblk{nblk} kind{kind}",
                    False, batch)
        batch.flush()
        v()


def test_reduce_batch_flushes():
    """8 items of mixed kinds, widths and row counts in one launch, three of them with a second partial array of a
    different row count; a single item with part_b (the multi kernel); a single item without (the single kernel)"""
    ops = ops_()
    items = [(33, 260, 0, False, 0), (1, 1, 0, True, 0), (129, 96, 2, False, 7), (4096, 31, 1, True, 0),
             (31, 32, 2, True, 0), (257, 33, 1, False, 300), (128, 260, 0, True, 1), (32, 4, 1, False, 0)]
    batch = ops.ReduceBatch()
    checks = []
    for i, (nblk, N, kind, acc, nb_b) in enumerate(items):
        assert len(batch.items) == i
        checks.append(run_csr(rc.csr_int_case(nblk, N, 200 + 5 * i, kind, acc, nb_b), f"flush8 item{i}", True, batch))
    assert len(batch.items) == 0        # the eighth add flushes
    for v in checks:
        v()
    for nb_b in (5, 0):
        v = run_csr(rc.csr_int_case(130, 96, 300, 2, True, nb_b), f"flush1 part_b={nb_b}", True, batch)
        assert len(batch.items) == 1
        batch.flush()
        v()
    part1 = rc.csr_int_case(37, 1, 310, 0, False)   # a 1-D partial array (the scalar sums): N = 1
    part1["part"] = part1["part"].reshape(-1)
    run_csr(part1, "colsum_reduce 1-D", True)()


def test_nblk_override_is_validated():
    ops = ops_()
    d = rc.row_case(3, 4, 1)
    x, w, g, sk = D(d["h"]), D(d["w"]), D(d["dout"]), D(d["skip1"])
    _, rstd = ops.rmsnorm_fwd(x, w, d["eps"])
    for bad in (0, 4097, -1):
        with pytest.raises(ValueError):
            ops.rmsnorm_bwd(g, x, w, rstd, nblk=bad)
        with pytest.raises(ValueError):
            ops.norm_skip_bwd(g, x, None, sk, nblk=bad)
        with pytest.raises(ValueError):
            ops.res_skip_bwd(modes()[0], g, x, x, sk, x, nblk=bad)
        with pytest.raises(ValueError):
            ops.res_rmsnorm_bwd(modes()[0], g, x, None, w, rstd, nblk=bad)
        with pytest.raises(ValueError):
            ops.lerp_bwd(modes()[0], g, x, x, D(d["alpha"]), d["c_a"], None, None, None, False, True, True, nblk=bad)
        with pytest.raises(ValueError):
            ops.qknorm_bwd(modes()[0], None, None, None, None, None, None, None, None, 1.0, g, 4, g, 4, g, 4, 1, 3, 1, 4,
                           nblk=bad)
