"""The MFMA attention kernels (impl 1, bf16) against the fp64 reference and the per-element bounds of attn_check.py,
through the padding harness (NaN operand margins, sentinel output margins): nvit_attn_fwd / nvit_attn_bwd (online path,
and the UNIT backward at scale = ln 2), nvit_attn_fwd_bounded (FAST, FAST + UNIT, and a bound over the limit that falls
back to the online path), at head dims 32, 64 and 128, on counting, two-level and Gaussian data, at equal and unequal
lengths, the training length, and the fused d = 64 backward nvit_attn_bwd_qknorm.  test_attn_check.py shows on the CPU
which kernel mistakes these cases and bounds expose.  Every test prints its largest err / bound."""
import math

import pytest
import torch

import attn_check as A

pytestmark = pytest.mark.gpu

B0, H0 = 2, 3


def _lib():
    from nvit_amd import _lib
    return _lib


def _check_case(c, backward, label):
    """forward (the entry and path the case is built for) and, for the generic entry, backward"""
    BF16 = _lib().BF16
    B, H, Tq, d = c["q"].shape
    Tk = c["k"].shape[2]
    ref = A.attn_ref(c, backward)
    o_tok, lse = A.run_fwd(BF16, 1, c["q"], c["k"], c["v"], c["scale"], c["sqk"], c["c_q"], c["qpre"])
    o = A.untok(o_tok.cpu(), B, H)
    got = {"o": o, "lse": lse.cpu()}
    bound = A.fwd_bounds(c, ref)
    if Tk == 1:      # one key: the output is v itself
        assert A.bits_equal(o.contiguous(), c["v"].expand(B, H, Tq, d).contiguous()), f"{label}: o != v at Tk = 1"
    if backward:
        assert c["qpre"] == 1.0 and c["sqk"] is None
        dq, dk, dv = A.run_bwd(BF16, 1, A.tok(c["g"]), c["q"], c["k"], c["v"], o_tok, lse, c["scale"])
        got.update(dq=dq.cpu(), dk=dk.cpu(), dv=dv.cpu())
        bound.update(A.bwd_bounds(c, ref, o, lse.cpu()))
        if Tk == 1:
            assert (got["dq"] == 0).all(), f"{label}: dq != 0 at Tk = 1"
    A.check_all(got, ref, bound, f"{label} {A.path_of(c)}")


def _run_configs(family, B, H, Tq, Tk, d, configs=A.CONFIGS):
    from nvit_amd import ops
    assert A.q_prescale(d) == ops.attn_q_prescale(d)
    for config in configs:
        c = A.make_case(family, config, B, H, Tq, Tk, d)
        assert A.path_of(c) == {"online": "online", "unit_bwd": "online", "fast": "fast", "fast_unit": "unit",
                                "over": "online"}[config]
        _check_case(c, config in ("online", "unit_bwd"), f"d={d} ({B},{H}) Tq={Tq} Tk={Tk} {family} {config}")


EQUAL = [(d, T, f) for d in A.HEAD_DIMS for T in A.equal_lengths(d) for f in A.FAMILIES if f != "gauss" or A.gauss_runs(T, T)]


@pytest.mark.parametrize("d,T,family", EQUAL)
def test_equal_lengths(d, T, family):
    """T covers every nkf / ns2 of the masked tile, a single live row in the second workgroup and a fourth tile that
    reuses ring slot 0 (KV tile 64 / 64 / 32 keys, 128 queries per workgroup, dK/dV 128 / 128 / 64 keys)."""
    _run_configs(family, B0, H0, T, T, d)


@pytest.mark.parametrize("d", A.HEAD_DIMS)
@pytest.mark.parametrize("B,H", [(1, 1), (3, 3)])
@pytest.mark.parametrize("family", ["counting_q", "counting_k", "two_level"])
def test_grid_sizes(d, B, H, family):
    """T = 129: grids of 2 and 18 workgroups (12 in test_equal_lengths) through the XCD re-deal of work_index"""
    _run_configs(family, B, H, 129, 129, d)


UNEQ = [(d, Tq, Tk, f) for d in A.HEAD_DIMS for (Tq, Tk) in A.UNEQUAL for f in A.FAMILIES
        if f != "gauss" or A.gauss_runs(Tq, Tk)]


@pytest.mark.parametrize("d,Tq,Tk,family", UNEQ)
def test_unequal_lengths(d, Tq, Tk, family):
    """Tq != Tk on every entry, forward and backward; Tk = 1 returns v itself and dq = 0"""
    _run_configs(family, B0, H0, Tq, Tk, d)


@pytest.mark.parametrize("family", ["counting_q", "counting_k"])
def test_training_length(family):
    """T = 784, d = 64: on counting data the bound is a twentieth of one key's weight (test_attn_check.py)"""
    _run_configs(family, 1, 2, 784, 784, 64, ("online", "fast", "fast_unit"))


# ------------------------------------------------------------------------------------------------ fused backward
@pytest.mark.parametrize("T", A.FUSED_T)
@pytest.mark.parametrize("prescale", [False, True])
@pytest.mark.parametrize("with_sqk", [True, False])
@pytest.mark.parametrize("layout", ["one_buffer", "separate"])
def test_fused_backward(T, prescale, with_sqk, layout):
    """nvit_attn_bwd_qknorm: dq | dk | dv token-major and d sqk (after colsum_reduce of part_q and part_k) against the
    fp64 head-major gradients pushed through qknorm_bwd_formula; the pre-scaled q takes the generated-assembly dK/dV
    loop (at its default).  separate: three buffers with ldq != ldkv whose columns beyond the C head columns hold a
    sentinel that must survive."""
    from nvit_amd import ops
    BF16 = _lib().BF16
    B, H, d = B0, H0, 64
    C, M = H * d, B * T
    qpre = ops.attn_q_prescale(d) if prescale else 1.0
    c = A.fused_case(B, H, T, 5, qpre, with_sqk)
    dv_ = A.dev()
    q, k, v = (c[n].to(dv_) for n in ("q", "k", "v"))
    g_tok = A.tok(c["g"]).to(dv_)
    sqk = c["sqk"].to(dv_) if with_sqk else None
    rq, rk = (c["rq"].to(dv_), c["rk"].to(dv_)) if with_sqk else (None, None)
    o, lse = ops.attn_fwd(BF16, 1, q, k, v, c["scale"], sqk, c["c_q"], q_prescale=qpre)
    if layout == "one_buffer":
        buf = torch.full((M, 3 * C), A.SENTINEL, device=dv_, dtype=torch.bfloat16)
        dq, dk, dv, ldq, ldkv = buf, buf[:, C:], buf[:, 2 * C:], 3 * C, 3 * C
        outs = {"dq": buf[:, :C], "dk": buf[:, C:2 * C], "dv": buf[:, 2 * C:]}
        extra = []
    else:
        ldq, ldkv = C + 8, C + 16
        dq = torch.full((M, ldq), A.SENTINEL, device=dv_, dtype=torch.bfloat16)
        dk, dv = (torch.full((M, ldkv), A.SENTINEL, device=dv_, dtype=torch.bfloat16) for _ in range(2))
        outs = {"dq": dq[:, :C], "dk": dk[:, :C], "dv": dv[:, :C]}
        extra = [dq[:, C:], dk[:, C:], dv[:, C:]]
    pq, pk = ops.attn_bwd_qknorm(g_tok, q, k, v, o, lse, c["scale"], rq, rk, sqk, c["c_q"], dq, ldq, dk, dv, ldkv,
                                 q_prescale=qpre)
    torch.cuda.synchronize()
    for x in extra:
        assert (x.float() == A.SENTINEL).all(), "columns beyond the head block were written"
    got = {n: t.cpu() for n, t in outs.items()}
    if with_sqk:
        rows = B * math.ceil(T / ops.ATTN_BWD_PART_ROWS)
        assert tuple(pq.shape) == (rows, C) and tuple(pk.shape) == (rows, C)
        assert torch.isfinite(pq).all() and torch.isfinite(pk).all()
        dsq = torch.empty(C, device=dv_)
        ops.colsum_reduce(pq, dsq, False, kind=0, scale=c["c_q"])
        ops.colsum_reduce(pk, dsq, True, kind=0, scale=c["c_q"])
        got["dsqk"] = dsq.cpu()
    else:
        assert pq is None and pk is None
    ref = A.attn_ref(c)
    hb = A.bwd_bounds(c, ref, A.untok(o.cpu(), B, H), lse.cpu())
    vals, bounds = A.fused_ref_bounds(c, ref, hb)
    A.check_all(got, vals, bounds, f"fused T={T} qpre={qpre:.2f} sqk={with_sqk} {layout}")
