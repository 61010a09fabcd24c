"""CPU: what the six row entry points refuse when a gate is given (include/nvit_hip.h, the "gate (optional)" paragraphs).
Every refusal is an argument check that returns before any HIP call, so nothing is launched and no device memory is
needed: the pointers are null or the address of a host buffer that is never read.  Each call must return non-zero and
leave an error text that names its entry point and the argument at fault.  The one `gpu` case asks
nvit_lerp_bwd_blocks, whose occupancy query answers only on a device."""
import ctypes

import pytest

F32, BF16 = 0, 1
M, C, T = 12, 64, 3          # a valid shape: C % 4 == 0, M a multiple of the T rows per sample
_HOST = ctypes.create_string_buffer(64)
PTR = ctypes.addressof(_HOST)

# argument names in the order of the C declarations
ARGS = {
    "nvit_lerp_fwd": "dt h y y_dt alpha c_a skip_x skip gate rows_per_sample out out_lo M C stream",
    "nvit_lerp_bwd": "dt dout dout_add h y y_dt alpha c_a skip_x skip gate rows_per_sample dh accum_dh dy dy_lo dskip_x "
                     "part_dlam part_dskip nblk M C stream",
    "nvit_res_rmsnorm_fwd": "dt a y y_dt w eps gate rows_per_sample out out_lo rstd M C stream",
    "nvit_res_rmsnorm_bwd": "dt g g_add a y y_dt w rstd gate rows_per_sample dz accum dz_lo part_dw nblk M C stream",
    "nvit_res_skip_fwd": "dt h y y_dt skip x gate rows_per_sample out out_lo M C stream",
    "nvit_res_skip_bwd": "dt dout h y y_dt skip x gate rows_per_sample dh dh_lo dx part_dskip nblk M C stream",
}
# what a gated call of the block chain passes: every operand present, the MLP half of lerp_bwd (skip_x without accum_dh)
SCALARS = {"dt": BF16, "y_dt": BF16, "c_a": 1.0, "eps": 1e-6, "rows_per_sample": T, "accum_dh": 0, "accum": 0, "nblk": 2,
           "M": M, "C": C, "stream": None}


def refused(name, **over):
    """calls `name` with a complete gated argument list changed by `over`; -> the error text of the refusal"""
    from nvit_amd import _lib
    lib = _lib.load()
    names = ARGS[name].split()
    assert len(names) == len(_lib.SIGNATURES[name]) and set(over) <= set(names), name
    vals = {n: SCALARS.get(n, PTR) for n in names}
    vals.update(over)
    rc = getattr(lib, name)(*[vals[n] for n in names])
    assert rc != 0, f"{name} accepted {over}"
    msg = lib.nvit_last_error().decode()
    assert msg.startswith(name[len("nvit_"):] + ":"), (name, msg)
    return msg


@pytest.mark.parametrize("name", sorted(ARGS))
def test_gate_needs_rows_per_sample_that_divide_the_rows(name):
    assert "rows_per_sample=0" in refused(name, rows_per_sample=0)
    assert "rows_per_sample=5" in refused(name, rows_per_sample=5)       # M = 12 is no multiple of 5


def test_lerp_bwd_with_a_gate_takes_skip_x_or_accum_dh_but_not_both_or_neither():
    for over in ({"accum_dh": 1}, {"skip_x": None, "accum_dh": 0}):
        msg = refused("nvit_lerp_bwd", **over)
        assert "skip_x" in msg and "accum_dh" in msg, msg


def test_res_rmsnorm_with_a_gate_needs_y_and_its_backward_the_addend():
    for name in ("nvit_res_rmsnorm_fwd", "nvit_res_rmsnorm_bwd"):
        assert "needs y" in refused(name, y=None)
    assert "g_add" in refused("nvit_res_rmsnorm_bwd", g_add=None)


@pytest.mark.gpu
def test_lerp_bwd_blocks_reports_no_grid_for_variants_with_a_gate_that_are_not_built():
    """on a device, where the occupancy query answers: the two built gated variants get a grid, the other two get 0"""
    from nvit_amd import _lib
    blocks = _lib.load().nvit_lerp_bwd_blocks
    for has_add in (0, 1):
        for has_skip, accum in ((1, 0), (0, 1)):
            assert blocks(BF16, BF16, C, has_add, has_skip, accum, 1) > 0
        for has_skip, accum in ((1, 1), (0, 0)):
            assert blocks(BF16, BF16, C, has_add, has_skip, accum, 0) > 0
            assert blocks(BF16, BF16, C, has_add, has_skip, accum, 1) == 0
