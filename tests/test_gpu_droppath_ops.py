"""GPU tests, op level, of stochastic depth: nvit_droppath_draw against its numpy twin (droppath_ref.draw) bit for bit,
and the six row kernels with a gate (nvit_lerp_* of the nViT blocks, nvit_res_rmsnorm_* and nvit_res_skip_* of the
plain-ViT blocks) through nvit_amd.ops - every width class, 1, 3 and 49 rows per sample with M no multiple of the rows
per workgroup, waves that walk rows of several samples (explicit nblk), a forward grid that wraps, fp32 and bf16 y and
copies, and the switch combinations the block chain launches - against: gates all 1 = the plain kernel's bits; gates all
0 = no gradient into the branch and the plain kernel's output at alpha = 0 (LERP) or y = 0 (residual); mixed gates inside
the fp64 element bounds of droppath_ref; and the same bounds REJECT the output when the reference is given the gate table
shifted by one sample (a wrong row -> sample index would be seen).  Run: pytest -m gpu."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import droppath_ref as dr
import rowops_check as rc

F32T, BF16T = torch.float32, torch.bfloat16
NAN = float("nan")
WIDTHS = [64, 192, 768, 1280, 2048]        # NV = 1, 1, 3, 8, 8 (192: a partly filled vector)
SAMPLES = {1: 7, 3: 5, 49: 3}              # rows per sample T -> B: M = 7, 15, 147, none a multiple of ROW_WAVES
GATE_VALUES = (0.0, 1.0, 1.0 / 0.9)


def dev():
    return torch.device("cuda:0")


def ops_():
    from nvit_amd import ops
    return ops


def modes():
    from nvit_amd import _lib
    return _lib.F32, _lib.BF16


def D(t):
    return None if t is None else t.to(dev())


def poison(*shape, dtype=F32T):
    return torch.full(shape, NAN, device=dev(), dtype=dtype)


def mixed_gates(B):
    """dropped, kept, kept and scaled, in turn: neighbouring samples always differ"""
    return torch.tensor([GATE_VALUES[b % 3] for b in range(B)], dtype=F32T)


def same_bits(a, b, label):
    if a is None or b is None:
        assert a is None and b is None, label
        return
    assert rc.bits_equal(a.cpu(), b.cpu()), f"{label}: differs from the plain kernel's bits"


# ------------------------------------------------------------------------------------------------ the draw
def make_dp(rate, seed, first_index, scale):
    from nvit_amd import DropPath
    return DropPath(rate, seed=seed, first_index=first_index, scale_by_keep=scale).to(dev())


@pytest.mark.parametrize("n_layer,B", [(1, 1), (2, 5), (12, 128), (32, 513)])
def test_draw_equals_the_numpy_twin(n_layer, B):
    for scale, rate, (seed, first, step) in itertools.product(
            (False, True), (0.1, 0.5), ((0, 0, 0), (2 ** 63 + 12345, 2 ** 32 + 77, 2 ** 35 + 3))):
        dp = make_dp(rate, seed, first, scale)
        dp.load_state_dict({"seed": seed, "step": step})
        t = dp.draw(n_layer, B)
        assert t.dtype == F32T and tuple(t.shape) == (2 * n_layer, B)
        want = dr.draw(seed, step, first, rate, n_layer, B, scale)
        assert np.array_equal(t.cpu().numpy().view(np.uint32), want.view(np.uint32)), (n_layer, B, scale, rate, seed)
        assert (t[:2] == 1.0).all()                       # p_0 = 0: the first block never drops
        assert dp.step == step + 1
        t2 = dp.draw(n_layer, B)                          # the counter advanced: the next step's table
        assert np.array_equal(t2.cpu().numpy(), dr.draw(seed, step + 1, first, rate, n_layer, B, scale))
        assert dp.step == step + 2


def test_draw_split_batch_and_values():
    dp = make_dp(0.5, 9, 0, True)
    whole = dp.draw(4, 8)
    parts = []
    for first in (0, 4):
        part = make_dp(0.5, 9, first, True)
        parts.append(part.draw(4, 4))                     # (a fresh object: the counter is back at 0)
    assert torch.equal(whole, torch.cat(parts, dim=1))
    keep = np.float32(1.0) - dr.rates(0.5, 4)
    for l in range(4):
        vals = set(np.unique(whole[2 * l:2 * l + 2].cpu().numpy()).tolist())
        assert vals <= {0.0, float(np.float32(1.0) / keep[l])}, (l, vals)
    big = make_dp(0.5, 1, 0, False).draw(2, 4096)         # 16384 gates: more than the 256 threads hold at once
    assert np.array_equal(big.cpu().numpy(), dr.draw(1, 0, 0, 0.5, 2, 4096, False))
    with pytest.raises(ValueError):
        dp.draw(4, 0)


# ------------------------------------------------------------------------------------------------ gated LERP
def run_gated(d, gate, T, dt, nblk, *, plain=False, alpha=None):
    """forward + backward through ops with `gate` (plain: the ungated entry points) -> dict of every output"""
    ops = ops_()
    M, C = d["h"].shape
    h, y, xs, skip = D(d["h"]), D(d["y"]), D(d["skip_x"]), D(d["skip"])
    al = D(d["alpha"] if alpha is None else alpha)
    kw = {} if plain else {"gate": D(gate)}
    out, out_lo = ops.lerp_fwd(dt, h, y, al, d["c_a"], skip_x=xs, skip=skip, want_lo=True, **kw)
    accum = d["old"] is not None
    dh0 = D(d["old"]).clone() if accum else poison(M, C)
    want_dy = d["dout_add"] is None
    dh, dy, dy_lo, dxs, part, pskip = ops.lerp_bwd(dt, D(d["dout"]), h, y, al, d["c_a"], xs, skip, dh0, accum, want_dy, True,
                                                   dout_add=D(d["dout_add"]), nblk=nblk, **kw)
    assert tuple(part.shape) == (4 * nblk, C)
    return {"out": out, "out_lo": out_lo, "dh": dh, "dy": dy, "dy_lo": dy_lo, "dskip_x": dxs, "part": part, "pskip": pskip}


def check_gated_case(C, T, dt, y_bf16, mlp_half, add, seed):
    ops = ops_()
    B = SAMPLES[T]
    M = B * T
    assert M % 4 != 0
    nblk = 1 if M < 64 else 2               # 4 or 8 waves over M rows: a wave walks rows of several samples
    assert any(len({m // T for m in ms}) > 1 for ms in rc.wave_visits(M, nblk))
    d = rc.row_case(M, C, seed, y_bf16=y_bf16, skip=mlp_half, add=add, accum=not mlp_half)
    label = f"gated lerp C{C} T{T} dt={dt} ybf16={y_bf16} mlp={mlp_half} add={add}"
    plain = run_gated(d, None, T, dt, nblk, plain=True)
    # 1. gates all 1.0f: the plain kernel's bits, every output
    ones = run_gated(d, torch.ones(B), T, dt, nblk)
    for k in plain:
        same_bits(ones[k], plain[k], f"{label} gate=1 {k}")
    # 2. gates all 0.0f: nothing flows into the branch, the stream is that of alpha = 0
    zeros = run_gated(d, torch.zeros(B), T, dt, nblk)
    for k in ("dy", "dy_lo", "part"):
        if zeros[k] is not None:
            assert torch.equal(zeros[k], torch.zeros_like(zeros[k])), f"{label} gate=0: {k} is not exactly zero"
    a0 = run_gated(d, None, T, dt, nblk, plain=True, alpha=torch.zeros(C))
    same_bits(zeros["out"], a0["out"], f"{label} gate=0 out")
    same_bits(zeros["out_lo"], a0["out_lo"], f"{label} gate=0 out_lo")
    # 3. mixed gates: every element inside the fp64-derived bound
    gate = mixed_gates(B)
    res = run_gated(d, gate, T, dt, nblk)
    rc.rounded_copy(res["out_lo"], res["out"], label + " out_lo")
    dalpha = poison(C)
    ops.colsum_reduce(res["part"], dalpha, False, kind=1, ref=D(d["alpha"]), scale=d["c_a"])
    got = {"out": res["out"], "dh": res["dh"], "dy": res["dy"] if res["dy"] is not None else res["dy_lo"], "dalpha": dalpha}
    if res["dy"] is not None:
        rc.rounded_copy(res["dy_lo"], res["dy"], label + " dy_lo")
    if mlp_half:
        dskip = poison(1)
        ops.colsum_reduce(res["pskip"], dskip, False)
        got.update(dskip_x=res["dskip_x"], dskip=dskip)
    _, bnd = dr.gated_lerp_bounds(d, gate, T)
    rc.check_all(got, dr.gated_lerp_eval(d, gate, T), bnd, label, verbose=False)
    # 4. the mutant: against the table shifted by one sample the same comparison must fail
    shifted = torch.roll(gate, 1)
    ok = dr.within(got, dr.gated_lerp_eval(d, shifted, T), dr.gated_lerp_bounds(d, shifted, T)[1])
    assert not ok["out"] and not ok["dh"] and not ok["dy"] and not ok["dalpha"], f"{label}: shifted gates pass {ok}"


@pytest.mark.parametrize("C", WIDTHS)
def test_gated_lerp_fwd_bwd(C):
    F32, BF16 = modes()
    seed = 50
    for T, (dt, y_bf16), mlp_half, add in itertools.product(SAMPLES, ((F32, False), (BF16, True)), (True, False),
                                                            (False, True)):
        check_gated_case(C, T, dt, y_bf16, mlp_half, add, seed)
        seed += 10


def test_gated_lerp_type_product():
    """y fp32 / bf16 x copies fp32 / bf16 (the two pairs the model does not use) at one shape per rows-per-sample"""
    F32, BF16 = modes()
    for T, (dt, y_bf16), mlp_half in itertools.product(SAMPLES, ((F32, True), (BF16, False)), (True, False)):
        check_gated_case(260, T, dt, y_bf16, mlp_half, not mlp_half, 300 + T)


@pytest.mark.parametrize("T", sorted(SAMPLES))
def test_gated_lerp_fwd_grid_wraps(T):
    """more rows than one sweep of the forward grid (ROW_GRID_MAX workgroups x ROW_WAVES rows, read from the launcher's
    header constants): the rows of the second sweep take the gates of their own samples"""
    ops = ops_()
    F32, BF16 = modes()
    sweep = ops.ROW_GRID_MAX * ops.ROW_WAVES
    B = sweep // T + 2
    while (B * T) % 4 == 0:
        B += 1
    M, C = B * T, 64
    assert M > sweep
    gate = mixed_gates(B)
    for dt, y_bf16, skip in ((F32, False, True), (BF16, True, False)):
        d = rc.row_case(M, C, 70 + T, y_bf16=y_bf16, skip=skip)
        d["dout"] = None
        h, y, alpha, xs, sk = (D(d[k]) for k in ("h", "y", "alpha", "skip_x", "skip"))
        out, out_lo = ops.lerp_fwd(dt, h, y, alpha, d["c_a"], skip_x=xs, skip=sk, gate=D(gate))
        rc.rounded_copy(out_lo, out, "gated lerp_fwd wrap out_lo")
        rc.check(out, dr.gated_lerp_eval(d, gate, T)["out"], dr.gated_lerp_bounds(d, gate, T)[1]["out"],
                 f"gated lerp_fwd M{M} T{T} dt={dt}", verbose=False)
        ok = dr.within({"out": out}, dr.gated_lerp_eval(d, torch.roll(gate, 1), T),
                       {"out": dr.gated_lerp_bounds(d, torch.roll(gate, 1), T)[1]["out"]})
        assert not ok["out"]
        ones, _ = ops.lerp_fwd(dt, h, y, alpha, d["c_a"], skip_x=xs, skip=sk, gate=torch.ones(B, device=dev()))
        plain, _ = ops.lerp_fwd(dt, h, y, alpha, d["c_a"], skip_x=xs, skip=sk)
        same_bits(ones, plain, f"gated lerp_fwd wrap T{T} gate=1")


# ------------------------------------------------------------------------------------------------ gated residual kernels
def case_shape(T):
    B = SAMPLES[T]
    M = B * T
    nblk = 1 if M < 64 else 2
    assert M % 4 != 0 and any(len({m // T for m in ms}) > 1 for ms in rc.wave_visits(M, nblk))
    return B, M, nblk


def run_res_rmsnorm(d, gate, dt, nblk, *, plain=False, y=None):
    ops = ops_()
    a, w = D(d["h"]), D(d["w"])
    y = D(d["y"] if y is None else y)
    kw = {} if plain else {"gate": D(gate)}
    out, out_lo, rstd = ops.res_rmsnorm_fwd(dt, a, y, w, d["eps"], want_lo=True, **kw)
    dz0 = D(d["old"]).clone() if d["old"] is not None else None
    dz, dz_lo, part = ops.res_rmsnorm_bwd(dt, D(d["dout"]), a, y, w, rstd, g_add=D(d["dout_add"]), dz=dz0, want_lo=True,
                                          nblk=nblk, **kw)
    return {"out": out, "out_lo": out_lo, "rstd": rstd, "dz": dz, "dz_lo": dz_lo, "part": part}


def run_res_skip(d, gate, dt, nblk, *, plain=False, y=None):
    ops = ops_()
    h, skip, x = D(d["h"]), D(d["skip1"]), D(d["x"])
    y = D(d["y"] if y is None else y)
    kw = {} if plain else {"gate": D(gate)}
    out, out_lo = ops.res_skip_fwd(dt, h, y, skip, x, want_lo=True, **kw)
    dh, dh_lo, dx, part = ops.res_skip_bwd(dt, D(d["dout"]), h, y, skip, x, want_lo=True, nblk=nblk, **kw)
    return {"out": out, "out_lo": out_lo, "dh": dh, "dh_lo": dh_lo, "dx": dx, "part": part}


def check_gated_residual(kind, C, T, dt, y_bf16, accum, seed):
    """the four checks of check_gated_case for res_rmsnorm (fwd + bwd with g_add, dz written or accumulated) or res_skip"""
    ops = ops_()
    F32, _ = modes()
    B, M, nblk = case_shape(T)
    tl = F32T if dt == F32 else BF16T
    label = f"gated {kind} C{C} T{T} dt={dt} ybf16={y_bf16} acc={accum}"
    if kind == "res_rmsnorm":
        d = rc.row_case(M, C, seed, y_bf16=y_bf16, add=True, accum=accum, g_add_dtype=tl)
        run, lo_of, evalf, boundf = run_res_rmsnorm, ("dz", "dz_lo"), dr.gated_res_rmsnorm_eval, dr.gated_res_rmsnorm_bounds
    else:
        d = rc.row_case(M, C, seed, y_bf16=y_bf16)
        run, lo_of, evalf, boundf = run_res_skip, ("dh", "dh_lo"), dr.gated_res_skip_eval, dr.gated_res_skip_bounds
    full, lo = lo_of
    plain = run(d, None, dt, nblk, plain=True)
    ones = run(d, torch.ones(B), dt, nblk)
    for k in plain:
        same_bits(ones[k], plain[k], f"{label} gate=1 {k}")
    zeros = run(d, torch.zeros(B), dt, nblk)
    assert torch.equal(zeros[lo], torch.zeros_like(zeros[lo])), f"{label} gate=0: {lo} is not exactly zero"
    y0 = run(d, None, dt, nblk, plain=True, y=torch.zeros_like(d["y"]))
    for k in ("out", "out_lo"):
        same_bits(zeros[k], y0[k], f"{label} gate=0 {k}")
    gate = mixed_gates(B)
    res = run(d, gate, dt, nblk)
    rc.rounded_copy(res["out_lo"], res["out"], label + " out_lo")
    got = {"out": res["out"], full: res[full], "dy": res[lo]}
    if kind == "res_rmsnorm":
        dw = poison(C)
        ops.colsum_reduce(res["part"], dw, False)
        got.update(rstd=res["rstd"], dw=dw)
    else:
        dskip = poison(1)
        ops.colsum_reduce(res["part"], dskip, False)
        got.update(dx=res["dx"], dskip=dskip)
    # the low-precision copy is gate * the fp32 gradient, rounded once
    want_lo = (res[full] * D(dr.gate_rows(gate, T))).to(tl)
    assert rc.bits_equal(res[lo].cpu(), want_lo.cpu()), f"{label}: {lo} is not gate * {full} rounded once"
    rc.check_all(got, evalf(d, gate, T), boundf(d, gate, T)[1], label, verbose=False)
    shifted = torch.roll(gate, 1)
    ok = dr.within(got, evalf(d, shifted, T), boundf(d, shifted, T)[1])
    assert not ok["out"] and not ok[full] and not ok["dy"], f"{label}: shifted gates pass {ok}"


@pytest.mark.parametrize("C", WIDTHS)
def test_gated_res_rmsnorm_and_res_skip(C):
    F32, BF16 = modes()
    seed = 500
    for T, (dt, y_bf16) in itertools.product(SAMPLES, ((F32, False), (BF16, True))):
        for accum in (False, True):
            check_gated_residual("res_rmsnorm", C, T, dt, y_bf16, accum, seed)
        check_gated_residual("res_skip", C, T, dt, y_bf16, False, seed + 5)
        seed += 10
    if C == 192:      # the two type pairs the model does not use
        for dt, y_bf16 in ((F32, True), (BF16, False)):
            check_gated_residual("res_rmsnorm", C, 3, dt, y_bf16, False, 700)
            check_gated_residual("res_skip", C, 3, dt, y_bf16, False, 705)


@pytest.mark.parametrize("T", sorted(SAMPLES))
def test_gated_residual_fwd_grid_wraps(T):
    ops = ops_()
    F32, BF16 = modes()
    sweep = ops.ROW_GRID_MAX * ops.ROW_WAVES
    B = sweep // T + 2
    while (B * T) % 4 == 0:
        B += 1
    M, C = B * T, 64
    gate = mixed_gates(B)
    shifted = torch.roll(gate, 1)
    for dt, y_bf16 in ((F32, False), (BF16, True)):
        d = rc.row_case(M, C, 80 + T, y_bf16=y_bf16)
        a, y, w, sk, x = (D(d[k]) for k in ("h", "y", "w", "skip1", "x"))
        out, out_lo, rstd = ops.res_rmsnorm_fwd(dt, a, y, w, d["eps"], gate=D(gate))
        rc.rounded_copy(out_lo, out, "gated res_rmsnorm_fwd wrap out_lo")
        ref, bnd = dr.gated_res_rmsnorm_eval(d, gate, T), dr.gated_res_rmsnorm_bounds(d, gate, T)[1]
        rc.check_all({"out": out, "rstd": rstd}, ref, {k: bnd[k] for k in ("out", "rstd")},
                     f"gated res_rmsnorm_fwd M{M} T{T}", verbose=False)
        assert not dr.within({"out": out}, dr.gated_res_rmsnorm_eval(d, shifted, T),
                             {"out": dr.gated_res_rmsnorm_bounds(d, shifted, T)[1]["out"]})["out"]
        out, out_lo = ops.res_skip_fwd(dt, a, y, sk, x, gate=D(gate))
        rc.rounded_copy(out_lo, out, "gated res_skip_fwd wrap out_lo")
        rc.check(out, dr.gated_res_skip_eval(d, gate, T)["out"], dr.gated_res_skip_bounds(d, gate, T)[1]["out"],
                 f"gated res_skip_fwd M{M} T{T}", verbose=False)
        assert not dr.within({"out": out}, dr.gated_res_skip_eval(d, shifted, T),
                             {"out": dr.gated_res_skip_bounds(d, shifted, T)[1]["out"]})["out"]


def test_gate_arguments_are_validated():
    ops = ops_()
    F32, _ = modes()
    d = rc.row_case(12, 64, 90, skip=True)
    h, y, alpha, xs, sk, g = (D(d[k]) for k in ("h", "y", "alpha", "skip_x", "skip", "dout"))
    on = lambda *s, **kw: torch.ones(*s, device=dev(), **kw)
    for bad in (on(5), on(4, dtype=torch.float64), on(2, 2), on(8)[::2]):   # no divisor of M, fp64, 2-D, strided
        with pytest.raises(ValueError):
            ops.lerp_fwd(F32, h, y, alpha, d["c_a"], gate=bad)
    with pytest.raises(ValueError):
        ops.lerp_fwd(F32, h, y, alpha, d["c_a"], gate=torch.ones(4))                      # a host tensor
    gate = torch.ones(4, device=dev())
    with pytest.raises(ValueError):                                                       # skip with accumulation
        ops.lerp_bwd(F32, g, h, y, alpha, d["c_a"], xs, sk, torch.zeros_like(h), True, False, True, gate=gate)
    with pytest.raises(ValueError):                                                       # neither
        ops.lerp_bwd(F32, g, h, y, alpha, d["c_a"], None, None, None, False, False, True, gate=gate)
    w = D(d["w"])
    with pytest.raises(ValueError):                                                       # no branch output to gate
        ops.res_rmsnorm_fwd(F32, h, None, w, d["eps"], gate=gate)
    _, _, rstd = ops.res_rmsnorm_fwd(F32, h, y, w, d["eps"], gate=gate)
    with pytest.raises(ValueError):                                                       # built with the addend only
        ops.res_rmsnorm_bwd(F32, g, h, y, w, rstd, gate=gate)
    with pytest.raises(ValueError):
        ops.res_skip_fwd(F32, h, y, sk, xs, gate=on(5))
    with pytest.raises(ValueError):
        ops.res_skip_bwd(F32, g, h, y, sk, xs, gate=on(5))
