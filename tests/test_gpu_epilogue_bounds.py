"""The four fused-epilogue launches of the persistent 256x256 NT GEMM against the fp64 oracles of epilogue_check.py:
nvit_gemm_nt_swiglu (EPI 3), nvit_gemm_nt_swiglu_act (EPI 6), nvit_gemm_nt_qknorm (EPI 4), each with and without a bias, and
nvit_gemm_nt_swiglu_bwd (EPI 5), called through the C entry points on buffers of this test.

Operands are exact integers (the accumulator entering the epilogue is known exactly), views inside NaN-filled buffers
with lda, ldb > K and NaN rows below; the saved uv of EPI 5 has NaN rows below it too.  Every output is pre-filled with
a NaN bit pattern and followed by guard rows that must be unchanged; an output the launch does not own (rq / rk of a
split-only or k-less launch, the head tensor of an absent part) must be unchanged as a whole.  Raw outputs (uv, vh,
split-only kh) must be ONE bf16 rounding of the accumulator, bit for bit; everything else is held element by element
to the Ev bounds, all elements of the edge cases and the rows of gemm_check.sample_rows in the many-rounds cases, where
every output is also bit-identical to the same launch cut into row slices that give each workgroup at most one tile.

Largest err / bound measured on the MI355X (pytest -s, 256 CUs), per launch and output, over all cases of this file,
against the fp64 reference.  The bound of a bf16 output is mostly its half ulp, so a correctly rounded one reaches
about 1; for those the second figure is the largest share of a case's elements that are not the rounded reference,
the third the fp32 error that those elements show (epilogue_check.crossed) over the fp32 part of the bound:

  launch  output            err / bound   not rounded ref.   fp32 error seen / fp32 bound
  EPI 3   uv                exact bits
  EPI 3   xm                1.000         0.00558            0.276
  EPI 6   xm                1.000         0.00558            0.276      (and the bits of EPI 3's xm in every case)
  EPI 4   vh, split kh      exact bits
  EPI 4   qh                0.999         0.00002            0.046
  EPI 4   kh                0.999         0.00004            0.038
  EPI 4   rq (fp32)         0.037
  EPI 4   rk (fp32)         0.036
  EPI 5   duv               1.000         0.00005            0.238
  EPI 5   part (fp32)       0.180                                       (dead rows exactly 0, none left NaN)
  EPI 5   dsuv (fp32)       0.219                                       (colsum_reduce of part)
  many rounds (EPI 3, 6, 5, and 4 at T = 256 and at T = 37) x (K 128 static, K 384 static, K 384 dynamic): every
  output buffer, guard rows included, exact bits of the row-sliced launches

(xm with gs off is where the 0.00558 and the 0.276 come from: the pre-activations are the raw integer sums, |v| reaches
about 100, and the argument of the fast exponential carries 2 |v| roundings.  The fp32 CPU emulation of the same form,
epilogue_check.swiglu_fwd_f32(c, fast=True), gives 0.0052 and 0.273 on data of that shape (M 300, F 384, K 320); some
of those elements are exact bf16 ties of u v, which the fp64 reference misses by a hair, and sit at err / bound =
1.000 by construction.)
No margin above 1 and no differing bit was found: the kernels are unchanged.
"""
import pytest
import torch

import epilogue_check as ec
import gemm_check as gc
import rowops_check as rc
from test_gpu_gemm import BF16, F32, Out, _bits, _check, dev, lib, paths, place

pytestmark = pytest.mark.gpu

DT_BF16 = 1                     # NVIT_BF16
NAN = float("nan")
MARGINS = {}                    # (launch, output) -> largest err / bound of this run


def ops_():
    from nvit_amd import ops
    return ops


def prescale():
    return ops_().attn_q_prescale(ec.HEAD)


def stream():
    return torch.cuda.current_stream().cuda_stream


def p(t):
    return None if t is None else t.data_ptr()


def D(t):
    return None if t is None else t.to(dev())


def out2d(rows, cols, dtype):
    """a contiguous [rows, cols] output (the fused launches fix their leading dimensions) + 3 guard rows, NaN pattern"""
    return Out(rows, cols, dtype, ld=cols)


def under_nan_rows(x, dtype):
    """x as the first rows of a contiguous buffer whose 5 further rows are NaN"""
    buf = torch.full((x.shape[0] + 5, x.shape[1]), NAN, dtype=dtype, device=dev())
    buf[:x.shape[0]].copy_(x.to(dtype))
    return buf[:x.shape[0]]


def untouched(o, label):
    torch.cuda.synchronize()
    assert torch.equal(_bits(o.buf), _bits(o.before)), f"{label}: an output the launch does not own was written"


def judge(launch, k, got, ref, bnd, label):
    """one output against its reference: exact bits (bnd None) or the bound; the figures are kept for `report`"""
    got = got.cpu()
    m = ec.check_or_exact(got, ref, bnd, f"{label} {k}")
    if m is None:
        MARGINS[(launch, k + " (raw)")] = None
        return
    new = [m] + ([ec.misrounded(got, ref), ec.crossed(got, ref, bnd)] if got.dtype == BF16 else [])
    MARGINS[(launch, k)] = [max(a, b) for a, b in zip(new, MARGINS.get((launch, k), new))]


def report(launch):
    """a bf16 output's err / bound is about 1 whenever it rounds right (the half ulp is most of the bound), so it also
    gets: the share of elements that are not the rounded reference, and the fp32 error those show over the fp32 bound"""
    for (l, k), m in sorted(MARGINS.items()):
        if l == launch:
            print(f"== {l} {k}: " + ("exact bits" if m is None else f"max err/bound {m[0]:.3f}" + (
                "" if len(m) == 1 else f"; at most {m[1]:.5f} of a case not the rounded reference, fp32 error seen / "
                                       f"fp32 bound {m[2]:.3f}")))


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8


# ------------------------------------------------------------------------------------------------ launches
class SwigluFwd:
    """operands of EPI 3 / 6 on the device, launched over rows [r0, r1) into outputs of the whole M"""

    def __init__(self, d):
        self.d, self.M, self.F, self.K = d, d["M"], d["F"], d["K"]
        self.A, self.B = place(d["A"], BF16), place(d["B"], BF16)
        self.gs = D(None if d["gs"] is None else ec.interleave(d["gs"], self.F).contiguous())
        self.bias = D(d["bias"])

    def outputs(self):
        return {"uv": out2d(self.M, 2 * self.F, BF16), "xm": out2d(self.M, self.F, BF16)}

    def launch(self, o, epi=3, r0=0, r1=None):
        r1 = self.M if r1 is None else r1
        A = self.A[r0:r1]
        if epi == 3:
            _check(lib().nvit_gemm_nt_swiglu(DT_BF16, p(A), A.stride(0), p(self.B), self.B.stride(0),
                                             p(o["uv"].view[r0:]), p(o["xm"].view[r0:]), r1 - r0, self.F, self.K,
                                             p(self.gs), self.d["gscale"], p(self.bias), stream()),
                   "nvit_gemm_nt_swiglu")
        else:
            _check(lib().nvit_gemm_nt_swiglu_act(DT_BF16, p(A), A.stride(0), p(self.B), self.B.stride(0),
                                                 p(o["xm"].view[r0:]), r1 - r0, self.F, self.K, p(self.gs),
                                                 self.d["gscale"], p(self.bias), stream()),
                   "nvit_gemm_nt_swiglu_act")

    def verify(self, o, launch, label, rows=None):
        c = ec.swiglu_fwd_c(self.d, rows)
        ref, bnd = ec.swiglu_fwd_ref(c)
        take = (lambda t: t.cpu()) if rows is None else (lambda t: t[rows.to(dev())].cpu())
        judge(launch, "xm", take(o["xm"].view), ref, bnd, label)
        if launch == "EPI3":
            judge(launch, "uv", take(o["uv"].view), c["acc"], None, label)


class SwigluBwd:
    def __init__(self, d):
        self.d, self.M, self.F, self.K = d, d["M"], d["F"], d["K"]
        self.A, self.B = place(d["A"], BF16), place(d["B"], BF16)
        self.uv = under_nan_rows(ec.interleave(d["uv"], self.F), BF16)
        self.gs = D(d["gs"])

    def outputs(self):
        o = {"duv": out2d(self.M, 2 * self.F, BF16)}
        if self.gs is not None:
            o["part"] = out2d(ec.part_blocks(self.M), 2 * self.F, F32)
        return o

    def launch(self, o, r0=0, r1=None):
        r1 = self.M if r1 is None else r1
        assert r0 % ec.TILE == 0
        A, uv = self.A[r0:r1], self.uv[r0:r1]
        part = o["part"].view[r0 // ec.PART_ROWS:] if "part" in o else None
        _check(lib().nvit_gemm_nt_swiglu_bwd(DT_BF16, p(A), A.stride(0), p(self.B), self.B.stride(0), p(uv),
                                             p(o["duv"].view[r0:]), p(part), r1 - r0, self.F, self.K, p(self.gs),
                                             self.d["gscale"], stream()), "nvit_gemm_nt_swiglu_bwd")

    def verify(self, o, label):
        """all elements; and colsum_reduce of part against d(suv)"""
        c = ec.swiglu_bwd_c(self.d)
        ref, bnd = ec.swiglu_bwd_ref(c)
        got = {"duv": ec.deinterleave(o["duv"].view.cpu(), self.F)}
        if "part" in o:
            got["part"] = o["part"].view.cpu()
            dsuv = torch.full((2 * self.F + 8,), rc.SENTINEL, device=dev())
            ops_().colsum_reduce(o["part"].view, dsuv[:2 * self.F], False)
            assert (dsuv[2 * self.F:] == rc.SENTINEL).all()
            got["dsuv"] = dsuv[:2 * self.F].cpu()
            bnd["dsuv"] = bnd["dsuv"] + rc.csr_bound(got["part"])
        else:
            assert set(ref) == {"duv"}
        for k in ref:
            judge("EPI5", k, got[k], ref[k], bnd[k], label)

    def verify_rows(self, o, label, rows):
        c = ec.swiglu_bwd_c(self.d, rows)
        ref, bnd = ec.swiglu_bwd_ref(c, nblk=ec.part_blocks(len(rows)))
        got = ec.deinterleave(o["duv"].view[rows.to(dev())].cpu(), self.F)
        judge("EPI5", "duv", got, ref["duv"], bnd["duv"], label)
        for t0 in (0, (self.M - 1) // ec.TILE * ec.TILE):        # the part rows of the first and of the last row tile
            c = ec.swiglu_bwd_c(self.d, torch.arange(t0, min(t0 + ec.TILE, self.M)))
            ref, bnd = ec.swiglu_bwd_ref(c)
            b0 = t0 // ec.PART_ROWS
            judge("EPI5", "part", o["part"].view[b0:b0 + 2], ref["part"], bnd["part"], f"{label} rows {b0}, {b0 + 1} of")
        assert torch.isfinite(o["part"].view).all(), f"{label}: a part row was left unwritten"


class QkFused:
    def __init__(self, d):
        self.d, self.M, self.K = d, d["M"], d["K"]
        self.Bsz, self.T, self.H = d["Bsz"], d["T"], d["H"]
        self.A, self.B = place(d["A"], BF16), place(d["B"], BF16)
        self.sqk, self.bias = D(d["sqk"]), D(d["bias"])
        self.have = set(range(d["part0"], d["part0"] + d["nparts"]))

    def outputs(self):
        o = {n: out2d(self.Bsz * self.H * self.T, ec.HEAD, BF16) for n in ("qh", "kh", "vh")}
        o.update({n: out2d(self.M, self.H, F32) for n in ("rq", "rk")})
        return o

    def launch(self, o, r0=0, r1=None):
        r1 = self.M if r1 is None else r1
        assert r0 % self.T == 0 and (r1 - r0) % self.T == 0
        A = self.A[r0:r1]
        h0 = r0 // self.T * self.H * self.T                # first row of batch r0 / T in the [B * H * T, 64] view
        _check(lib().nvit_gemm_nt_qknorm(DT_BF16, p(A), A.stride(0), p(self.B), self.B.stride(0), r1 - r0, self.K,
                                         self.d["nparts"], self.d["part0"], p(self.sqk), self.d["c_q"], prescale(),
                                         p(o["qh"].view[h0:]), p(o["kh"].view[h0:]), p(o["vh"].view[h0:]),
                                         p(o["rq"].view[r0:]), p(o["rk"].view[r0:]), self.T, self.H, ec.HEAD,
                                         p(self.bias), stream()), "nvit_gemm_nt_qknorm")

    def verify(self, o, label, rows=None):
        c = ec.qk_fused_c(self.d, rows)
        ref, bnd = ec.qk_fused_ref(c, prescale())
        B, T, H = self.Bsz, self.T, self.H
        got = {}
        for k in o:
            if k not in ref:
                untouched(o[k], f"{label} {k}")
                continue
            t = o[k].view
            if k.endswith("h"):
                t = t.reshape(B, H, T, ec.HEAD)
                if rows is not None:        # the sampled rows as one batch of len(rows) tokens
                    t = t.permute(0, 2, 1, 3).reshape(B * T, H, ec.HEAD)[rows.to(dev())].permute(1, 0, 2)[None]
            elif rows is not None:
                t = t[rows.to(dev())]
            got[k] = t.cpu()
        assert set(got) == set(ref) == set(bnd)
        for k in ref:
            judge("EPI4", k, got[k], ref[k], bnd[k], label)


def guards(o, label):
    for k, out in o.items():
        out.assert_guard(f"{label} {k}")


# ------------------------------------------------------------------------------------------------ edge shapes
@pytest.mark.parametrize("M", ec.EDGE_M)
def test_swiglu_fwd_edges(M):
    """EPI 3 and EPI 6 at the row edges of the fragment, wave tile and tile; EPI 6's xm is the bits of EPI 3's"""
    cases = [(F, K, gs, 0) for F, K in ec.SWIGLU_FK for gs in (True, False)]
    cases += [(F, K, gs, launch) for launch, (Mb, F, K, gs) in ec.SWIGLU_BIAS.items() if Mb == M]
    for i, (F, K, gs, biased) in enumerate(cases):
        run = SwigluFwd(ec.swiglu_fwd_case(M, F, K, 1000 + 10 * i + M, gs, bias=bool(biased)))
        label = f"M{M} F{F} K{K} gs={gs} bias={bool(biased)}"
        xm = {}
        for epi in (3, 6):
            o = run.outputs()
            run.launch(o, epi)
            guards(o, f"EPI{epi} {label}")
            if epi == 6:
                untouched(o.pop("uv"), f"EPI6 {label} uv")
            run.verify(o, f"EPI{epi}", f"EPI{epi} {label}")
            xm[epi] = o["xm"].view
        assert gc.bits_equal(xm[3], xm[6]), f"{label}: the gate-only launch writes other bits than the full one"
    report("EPI3")
    report("EPI6")


@pytest.mark.parametrize("M", ec.EDGE_M)
def test_swiglu_bwd_edges(M):
    """EPI 5: duv, every part row (the dead ones exactly zero, none left NaN) and the reduced d(suv)"""
    for i, (F, K) in enumerate(ec.BWD_FK):
        for gs in (True, False):
            run = SwigluBwd(ec.swiglu_bwd_case(M, F, K, 2000 + 10 * i + M, gs))
            label = f"EPI5 M{M} F{F} K{K} gs={gs}"
            o = run.outputs()
            assert ("part" in o) == gs
            run.launch(o)
            guards(o, label)
            run.verify(o, label)
    report("EPI5")


@pytest.mark.parametrize("case", ec.QK_CASES, ids=ec.qk_id)
def test_qk_fused_edges(case):
    Bsz, T, H, K, nparts, part0, norm, bias = case
    run = QkFused(ec.qk_fused_case(Bsz, T, H, K, nparts, part0, 3000 + Bsz + T, norm, bias))
    label = "EPI4 " + ec.qk_id(case)
    o = run.outputs()
    run.launch(o)
    guards(o, label)
    run.verify(o, label)
    report("EPI4")


# ------------------------------------------------------------------------------------------------ many rounds
def rounds(make, T=None):
    """One launch over about 2.25 tiles per workgroup (K = 128 static; K = 384 static and dynamic) must write, in every
    output, the bits of the same launch cut into row slices of whole tiles that give each workgroup at most one tile;
    `make(M, K)` -> (runner, verify_rows).  The sampled rows are then held to the bounds."""
    n = n_cu()
    M, sl = ec.rounds_shape(n, T)
    assert -(-M // ec.TILE) * 4 > 2 * n and sl // ec.TILE * 4 <= n
    rows = gc.sample_rows(M)
    sliced = {}
    for K, dyn in ec.ROUNDS_K:
        if K not in sliced:
            run, verify_rows, label = make(M, K)
            with paths(sched=0):
                ref_o = run.outputs()
                for r0 in range(0, M, sl):
                    run.launch(ref_o, r0=r0, r1=min(r0 + sl, M))
            guards(ref_o, f"{label} sliced")
            verify_rows(run, ref_o, f"{label} K{K} sliced", rows)
            sliced[K] = (run, ref_o, label)
        run, ref_o, label = sliced[K]
        o = run.outputs()
        with paths(sched=dyn):
            run.launch(o)
            torch.cuda.synchronize()
        for k in o:
            assert gc.bits_equal(o[k].buf, ref_o[k].buf), \
                f"{label} K{K} sched={dyn} {k}: one launch over {-(-M // ec.TILE) * 4} tiles differs from its row slices"
        print(f"   {label} M{M} K{K} sched={dyn}: " + ", ".join(o) + " bit-identical to the row slices")
        if dyn:
            del sliced[K]


def test_swiglu_fwd_many_rounds():
    def make(M, K):
        return SwigluFwd(ec.swiglu_fwd_case(M, 512, K, 4000 + K)), \
            (lambda run, o, label, rows: run.verify(o, "EPI3", label, rows)), "EPI3 rounds"
    rounds(make)
    report("EPI3")


def test_swiglu_act_many_rounds():
    class Act(SwigluFwd):
        def outputs(self):
            return {"xm": out2d(self.M, self.F, BF16)}

        def launch(self, o, r0=0, r1=None):
            SwigluFwd.launch(self, o, 6, r0, r1)

    def make(M, K):
        return Act(ec.swiglu_fwd_case(M, 512, K, 4000 + K)), \
            (lambda run, o, label, rows: run.verify(o, "EPI6", label, rows)), "EPI6 rounds"
    rounds(make)
    report("EPI6")


def test_swiglu_bwd_many_rounds():
    def make(M, K):
        return SwigluBwd(ec.swiglu_bwd_case(M, 1024, K, 5000 + K)), \
            (lambda run, o, label, rows: run.verify_rows(o, label, rows)), "EPI5 rounds"
    rounds(make)
    report("EPI5")


@pytest.mark.parametrize("T", [256, ec.ROUNDS_QK_T])
def test_qk_fused_many_rounds(T):
    """T = 256: slices of whole tiles are whole batches (M a multiple of T: no ragged tile); T = 37: a ragged last
    tile, several batch crossings per wave tile, slices of 37 row tiles."""
    def make(M, K):
        return QkFused(ec.qk_fused_case(M // T, T, 8, K, 2, 0, 6000 + K + T)), \
            (lambda run, o, label, rows: run.verify(o, label, rows)), f"EPI4 rounds T{T}"
    rounds(make, T)
    report("EPI4")
