"""The GEMM oracles of gemm_check.py have teeth (CPU only, no GPU): a correct fp32 product in another summation order
passes both, and emulations of the ways a GEMM kernel goes wrong at its edges fail them."""
import pytest
import torch

import gemm_check as gc


def fp32_nt(A, B, bias=None, colscale=None, rowadd=None, period=0, old=None):
    """A correct kernel in fp32 (CPU matmul: another summation order than the fp64 reference)."""
    out = A.float() @ B.float().t()
    if bias is not None:
        out = out + bias
    if colscale is not None:
        out = out * colscale
    if rowadd is not None:
        out = out + rowadd[torch.arange(A.shape[0]) % period]
    if old is not None:
        out = out + old
    return out


def fails(fn):
    with pytest.raises(AssertionError):
        fn()


# ------------------------------------------------------------------------------------------ must pass
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
def test_exact_nt_fp32_matmul_is_bit_identical(out_dtype):
    d = gc.nt_exact(129, 136, 3072, seed=1, bias=True, colscale=True, period=7)
    ref, _ = gc.nt_ref(d["A"], d["B"], None, d["bias"], d["colscale"], d["rowadd"], 7)
    gc.assert_exact(fp32_nt(d["A"], d["B"], d["bias"], d["colscale"], d["rowadd"], 7).to(out_dtype), ref, "nt K=3072")


def test_exact_tn_fp32_matmul_is_bit_identical():
    d = gc.tn_exact(20000, 64, 72, seed=2)
    ref, _ = gc.tn_ref(d["A"], d["B"], 20000)
    # split sums reduced afterwards, as the kernels do
    parts = [d["A"][s:s + 6016].t() @ d["B"][s:s + 6016] for s in range(0, 20000, 6016)]
    gc.assert_exact(sum(parts[1:], parts[0]), ref, "tn Mred=20000")
    gc.assert_exact(d["A"].t() @ d["B"], ref, "tn Mred=20000 one sum")


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
def test_gauss_fp32_matmul_within_bound(out_dtype):
    A, B = gc.gauss_data((129, 3072), 3), gc.gauss_data((136, 3072), 4)
    bias, cs, radd = gc.gauss_data((136,), 5), gc.gauss_data((136,), 6), gc.gauss_data((7, 136), 7)
    ref, mag = gc.nt_ref(A, B, None, bias, cs, radd, 7)
    m = gc.check_gauss(fp32_nt(A, B, bias, cs, radd, 7).to(out_dtype), ref, mag, 3072, f"cpu nt K=3072 {out_dtype}")
    assert m > 0
    A, B = gc.gauss_data((20000, 64), 8), gc.gauss_data((20000, 72), 9)
    ref, mag = gc.tn_ref(A, B, 20000)
    gc.check_gauss(A.t() @ B, ref, mag, 20000 + 1, "cpu tn Mred=20000")


def test_sample_rows_covers_tile_edges():
    rows = gc.sample_rows(10241)
    s = set(rows.tolist())
    assert set(range(256)) <= s and set(range(10240, 10241)) <= s
    assert all(t in s and min(t + 256, 10241) - 1 in s for t in range(0, 10241, 256))
    assert gc.sample_rows(1000) is None


def test_exact_signed_zero_and_nan():
    ref = torch.tensor([[-0.0, 3.0]], dtype=torch.float64)
    gc.assert_exact(torch.tensor([[0.0, 3.0]]), ref, "+0 for -0")
    fails(lambda: gc.assert_exact(torch.tensor([[float("nan"), 3.0]]), ref, "nan"))
    fails(lambda: gc.assert_exact(torch.tensor([[0.0, float("nan")]]).bfloat16(), ref, "nan bf16"))


def test_exact_constructor_refuses_out_of_range():
    with pytest.raises(ValueError):
        gc.nt_exact(4, 4, 2 ** 20, seed=0)                # 2^20 * 16 = 2^24
    with pytest.raises(ValueError):
        gc.tn_exact(1 << 20, 8, 8, seed=0)
    with pytest.raises(ValueError):
        gc.require_exact(2 ** 20 - 1, 4, 4, addend=16)
    gc.require_exact(2 ** 20 - 1, 4, 4, addend=15)


# ------------------------------------------------------------------------------------------ must fail
def test_fault_missing_k_slab():
    d = gc.nt_exact(129, 129, 768, seed=10)
    A, B = d["A"], d["B"]
    ref, _ = gc.nt_ref(A, B)
    out = fp32_nt(A, B)
    out[128:, :128] -= A[128:, 64:128] @ B[:128, 64:128].t()     # one 64-wide slab lost in tile (1, 0)
    fails(lambda: gc.assert_exact(out, ref, "slab"))


def _tn_split_parts(A, B, Mred, splits, rb=64):
    rps = (Mred + splits - 1) // splits
    rps = (rps + rb - 1) // rb * rb                      # rows per split, as nvit_gemm_tn rounds them
    return rps, [A[s * rps:min((s + 1) * rps, Mred)].t() @ B[s * rps:min((s + 1) * rps, Mred)] for s in range(splits)]


def test_fault_tn_ragged_slab_dropped():
    d = gc.tn_exact(9001, 128, 136, seed=11)
    A, B = d["A"], d["B"]
    ref, _ = gc.tn_ref(A, B, 9001)
    rps, parts = _tn_split_parts(A, B, 9001, 3)
    last = 2 * rps + (9001 - 2 * rps) // 64 * 64        # first row of the last split's ragged slab
    assert 0 < 9001 - last < 64
    parts[2] = A[2 * rps:last].t() @ B[2 * rps:last]
    fails(lambda: gc.assert_exact(sum(parts[1:], parts[0]), ref, "ragged slab"))


def test_fault_tn_split_slab_garbage():
    d = gc.tn_exact(4160, 256, 256, seed=12)
    A, B = d["A"], d["B"]
    ref, _ = gc.tn_ref(A, B, 4160)
    rps, parts = _tn_split_parts(A, B, 4160, 64)
    assert parts[40].abs().max() == 0                   # trailing splits are empty
    gc.assert_exact(sum(parts[1:], parts[0]), ref, "all splits")
    parts[40] = gc.gauss_data((256, 256), 13)           # an empty split that never wrote its slab
    fails(lambda: gc.assert_exact(sum(parts[1:], parts[0]), ref, "garbage slab"))


def test_fault_bf16_truncated():
    d = gc.nt_exact(255, 129, 768, seed=14)
    ref, _ = gc.nt_ref(d["A"], d["B"])
    out = fp32_nt(d["A"], d["B"])
    trunc = (out.view(torch.int32) & ~0xFFFF).view(torch.float32).bfloat16()
    gc.assert_exact(out.bfloat16(), ref, "rounded")
    fails(lambda: gc.assert_exact(trunc, ref, "truncated"))


def test_fault_bf16_accumulate_double_rounding():
    d = gc.nt_exact(257, 1032, 448, seed=15, old_amax=448 * 16 * 1.1)
    ref0, _ = gc.nt_ref(d["A"], d["B"])
    old = gc.cancelling_old(ref0, seed=16).bfloat16()
    ref, _ = gc.nt_ref(d["A"], d["B"], old=old.float())
    prod = fp32_nt(d["A"], d["B"])
    gc.assert_exact((prod + old.float()).bfloat16(), ref, "one rounding")
    twice = (prod.bfloat16().float() + old.float()).bfloat16()   # product rounded to bf16 first, then "+= old"
    fails(lambda: gc.assert_exact(twice, ref, "double rounding"))


def test_fault_bias_after_colscale():
    d = gc.nt_exact(129, 127, 192, seed=17, bias=True, colscale=True)
    ref, _ = gc.nt_ref(d["A"], d["B"], None, d["bias"], d["colscale"])
    out = fp32_nt(d["A"], d["B"]) * d["colscale"] + d["bias"]
    fails(lambda: gc.assert_exact(out, ref, "epilogue order"))


def test_fault_rowadd_row_shifted():
    d = gc.nt_exact(129, 136, 192, seed=18, period=7)
    ref, _ = gc.nt_ref(d["A"], d["B"], None, None, None, d["rowadd"], 7)
    out = fp32_nt(d["A"], d["B"]) + d["rowadd"][(torch.arange(129) + 1) % 7]
    fails(lambda: gc.assert_exact(out, ref, "rowadd row"))


def test_fault_tail_column_duplicated():
    Bx = gc.int_data((130, 768), 4, seed=19)             # row 129 = the memory after the operand's last row
    d = gc.nt_exact(129, 129, 768, seed=20)
    ref, _ = gc.nt_ref(d["A"], Bx[:129])
    out = d["A"] @ Bx.t()
    out = torch.cat([out[:, :128], out[:, 129:130]], dim=1)   # column 129 stored into the last column 128
    fails(lambda: gc.assert_exact(out, ref, "tail column"))


def test_fault_gauss_operands_rounded_to_bf16():
    A, B = gc.gauss_data((256, 768), 21), gc.gauss_data((129, 768), 22)
    ref, mag = gc.nt_ref(A, B)
    gc.check_gauss(A @ B.t(), ref, mag, 768, "fp32 operands")
    out = A.bfloat16().float() @ B.bfloat16().float().t()
    fails(lambda: gc.check_gauss(out, ref, mag, 768, "bf16-rounded operands"))
    A, B = gc.gauss_data((20000, 64), 23), gc.gauss_data((20000, 72), 24)
    ref, mag = gc.tn_ref(A, B, 20000)
    fails(lambda: gc.check_gauss(A.bfloat16().float().t() @ B.bfloat16().float(), ref, mag, 20001, "tn bf16-rounded"))


def test_gauss_catches_missing_slab():
    A, B = gc.gauss_data((129, 768), 25), gc.gauss_data((129, 768), 26)
    ref, mag = gc.nt_ref(A, B)
    out = A @ B.t()
    out[128:, :128] -= A[128:, 64:128] @ B[:128, 64:128].t()
    fails(lambda: gc.check_gauss(out, ref, mag, 768, "slab"))
