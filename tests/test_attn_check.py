"""The attention oracles of attn_check.py checked on the CPU: the two statements of the fp64 gradients agree; the
emulator of the kernels' arithmetic - every path, both summation orders, every data family - lies inside every bound at
every shape of the GPU test; every mutant of the emulator exceeds a bound by a factor of 2 or more at every shape it
applies to, on a family that runs there; the counting family refuses a case outside its exact range and its bound stays
far below one key's weight at the training length; and a single wrong element anywhere is seen."""
import math

import pytest
import torch

import attn_check as A

B, H = 1, 2          # (the GPU test runs (2, 3); the head index is what the mutants need)


def shapes(d):
    return [(T, T) for T in A.equal_lengths(d)] + A.UNEQUAL


def families_at(Tq, Tk):
    return [f for f in A.FAMILIES if f != "gauss" or A.gauss_runs(Tq, Tk)]


@pytest.mark.parametrize("family,config", [("gauss", "online"), ("gauss", "fast_unit"), ("two_level", "unit_bwd"),
                                           ("counting_q", "fast"), ("counting_k", "online")])
@pytest.mark.parametrize("Tq,Tk", [(17, 17), (33, 129), (200, 1)])
def test_gradient_restatement(family, config, Tq, Tk):
    """autograd of the fp64 forward against the explicit dS formula: two fp64 evaluations of the same function lie
    within bound * U64 / U32 of each other (rowops_check.close_values)."""
    c = A.make_case(family, config, 2, 3, Tq, Tk, 32)
    ref, f = A.attn_ref(c), A.attn_grads_formula(c)
    b = A.all_bounds(c, ref, ref["o"], ref["lse"])
    for n in A.OUTS:
        tol = 2 * (b[n] + 1e-300) * (2.0 ** -53 / A.U32) + 2.0 ** -50 * ref[n].abs()
        assert ((ref[n] - f[n]).abs() <= tol).all(), n


@pytest.mark.parametrize("d", A.HEAD_DIMS)
def test_emulator_inside_bounds(d):
    worst = {}
    for Tq, Tk in shapes(d):
        for family in families_at(Tq, Tk):
            for config in A.CONFIGS:
                c = A.make_case(family, config, B, H, Tq, Tk, d)
                ref = A.attn_ref(c)
                for tiled in (True, False):
                    e = A.emulate(c, None, tiled)
                    m = A.margins(e, ref, A.all_bounds(c, ref, e["o_h"], e["lse_h"]))
                    for n, v in m.items():
                        key = (family, A.path_of(c) if n in ("o", "lse") else "bwd", n)
                        worst[key] = max(worst.get(key, 0.0), v)
                    assert max(m.values()) <= 1.0, (d, Tq, Tk, family, config, tiled, m)
    for key, v in sorted(worst.items()):
        print(f"   d={d} {key[0]:<11} {key[1]:<6} {key[2]:<3}: max err/bound {v:.3f}")


def test_emulator_paths_differ():
    """the switches switch: on Gaussian data the three paths give different bits, and so do the two summation orders
    of the online path (on the FAST paths the row sums are sums of bf16 values, exact in fp32 at this length)"""
    c = A.make_case("gauss", "fast", B, H, 129, 129, 64)     # (q not pre-scaled: the UNIT arithmetic drops a real factor)
    same = lambda x, y: A.bits_equal(x[0], y[0]) and A.bits_equal(x[1], y[1])
    outs = [A.emulate_fwd(c, p, True) for p in ("online", "fast", "unit")]
    assert not same(outs[0], outs[1]) and not same(outs[0], outs[2]) and not same(outs[1], outs[2])
    assert not same(outs[0], A.emulate_fwd(c, "online", False))


def _mutant_margins(cache, family, config, Tq, Tk, d, mutant):
    if (family, config) not in cache:
        c = A.make_case(family, config, B, H, Tq, Tk, d)
        ref = A.attn_ref(c)
        e = A.emulate(c)
        cache[(family, config)] = (c, ref, A.all_bounds(c, ref, e["o_h"], e["lse_h"]))
    c, ref, b = cache[(family, config)]
    return A.margins(A.emulate(c, mutant=mutant), ref, b)


@pytest.mark.parametrize("d", A.HEAD_DIMS)
def test_mutants_exceed_bounds(d):
    """online: the generic entry, forward and backward.  The mutants of the key loop are also shown on the forward of
    the FAST path.  h_dk_scale needs a pre-scaled q: the fused backward's shapes at d = 64."""
    seen = set()
    for Tq, Tk in shapes(d):
        cache = {}
        for mutant in A.MUTANTS:
            if mutant == "h_dk_scale" or not A.mutant_applies(mutant, H, Tq, Tk, d):
                continue
            configs = ["online"] + (["fast"] if mutant[0] in "abce" else [])
            for config in configs:
                res = {}
                for family in A.MUTANT_FAMILIES[mutant]:
                    if family in families_at(Tq, Tk):
                        m = _mutant_margins(cache, family, config, Tq, Tk, d, mutant)
                        res[family] = max(m[n] for n in (("o", "lse") if config == "fast" else A.OUTS))
                best = max(res.values())
                print(f"   d={d} Tq={Tq} Tk={Tk} {config:<6} {mutant:<20}: err/bound " +
                      ", ".join(f"{f} {v:.1f}" for f, v in res.items()))
                if (mutant, Tq, Tk) in A.NOT_SHOWN:
                    seen.add((mutant, Tq, Tk))
                    assert best < 2.0, "listed as not shown, but it is"
                else:
                    assert best >= 2.0, (d, Tq, Tk, config, mutant, res)
    assert seen == set(A.NOT_SHOWN)


@pytest.mark.parametrize("T", A.FUSED_T)
def test_mutant_dk_scale(T):
    d, mutant = 64, "h_dk_scale"
    assert A.mutant_applies(mutant, H, T, T, d, A.q_prescale(d)) and not A.mutant_applies(mutant, H, T, T, d, 1.0)
    res = {}
    for family in A.MUTANT_FAMILIES[mutant]:
        res[family] = _mutant_margins({}, family, "fast_unit", T, T, d, mutant)["dk"]
    print(f"   T={T} {mutant}: err/bound " + ", ".join(f"{f} {v:.1f}" for f, v in res.items()))
    assert max(res.values()) >= 2.0


def test_counting_guard_and_sharpness():
    A.require_counting_exact(784, 784, 64, 4)
    with pytest.raises(ValueError):
        A.require_counting_exact(2 ** 14, 2 ** 14, 64, 4)          # sum |v| could reach 2^16
    with pytest.raises(ValueError):
        A.counting_case(1, 1, 8, 2 ** 14, 32, 0)
    with pytest.raises(ValueError):
        A.require_counting_exact(8, 8, 128, 512)                   # a sum over d could reach 2^24
    # the training length: the forward bound (without the output's half ulp) is below a tenth of the weight 1 / Tk of
    # one key times the smallest |v| = 1, on the online and on the FAST path; every v and dO is a nonzero integer
    for config in ("online", "fast", "fast_unit"):
        c = A.make_case("counting_q", config, 1, 2, 784, 784, 64)
        assert (c["v"] != 0).all() and (c["g"] != 0).all() and (c["v"].float() == c["v"].float().round()).all()
        ref = A.attn_ref(c, backward=False)
        b = A.fwd_bounds(c, ref)
        print(f"   counting T=784 {config}: largest forward bound {b['o'].max().item():.2e} (one key: {1 / 784:.2e})")
        assert b["o"].max().item() < 0.1 / 784


def test_every_element_is_checked():
    """one element off by three bounds (and three half ulps) at the first, the last and a middle position of every
    output fails `check`; untouched outputs pass"""
    c = A.make_case("gauss", "online", B, H, 33, 65, 32)
    ref = A.attn_ref(c)
    e = A.emulate(c)
    b = A.all_bounds(c, ref, e["o_h"], e["lse_h"])
    A.check_all({n: e[n] for n in A.OUTS}, ref, b, "emulator", verbose=False)
    for n in A.OUTS:
        for pos in (0, e[n].numel() // 2, e[n].numel() - 1):
            bad = e[n].clone()
            full = b[n].reshape(-1)[pos] + A.half_ulp_bf16(ref[n].abs() + b[n]).reshape(-1)[pos]
            bad.view(-1)[pos] = (ref[n].reshape(-1)[pos] + 3 * full).to(bad.dtype)
            with pytest.raises(AssertionError):
                A.check(bad, ref[n], b[n], n, verbose=False)


def test_tk_one_returns_v():
    c = A.make_case("two_level", "online", B, H, 200, 1, 64)
    e = A.emulate(c)
    assert A.bits_equal(e["o"], c["v"].expand(B, H, 200, 64).contiguous())
    assert (e["dq"] == 0).all()
    assert math.isclose(A.two_level_a(257, 64, 8.0, 0) ** 2 * 8.0, math.log(63), rel_tol=0.02)


@pytest.mark.parametrize("qpre", [1.0, A.q_prescale(64)])
@pytest.mark.parametrize("with_sqk", [True, False])
def test_fused_backward_bounds(qpre, with_sqk):
    """the fused backward's oracle: the Ev run's values are the float64 formula, and the emulator's fp32 accumulators
    pushed through the formula in fp32 and rounded to bf16 lie inside the bounds"""
    from rowops_check import close_values
    c = A.fused_case(1, 2, 49, 5, qpre, with_sqk)
    ref = A.attn_ref(c)
    o, lse = A.emulate_fwd(c)
    hb = A.bwd_bounds(c, ref, o, lse)
    vals, bounds = A.fused_ref_bounds(c, ref, hb)
    dq, dk, dv = A.emulate_bwd(c, o, lse, raw=True)
    B_, H_, T, d = c["q"].shape
    fh = lambda t: A.from_heads(t, B_, T, H_, d)
    if with_sqk:
        close_values(A.fused_values_f64(c, ref), bounds, vals, "fused")
        cc = {"sqk": c["sqk"], "c_q": c["c_q"], "B": B_, "T": T, "H": H_, "d": d, "gq": dq, "gk": dk}
        fwd = {"qh": c["q"].float() * (1.0 / torch.tensor(qpre, dtype=torch.float32)), "kh": c["k"].float(),
               "rq": c["rq"], "rk": c["rk"]}
        res = A.qknorm_bwd_formula(cc, fwd, torch.float32)
        got = {"dq": res["dq"].bfloat16(), "dk": res["dk"].bfloat16(), "dv": fh(dv).bfloat16(), "dsqk": res["dsqk"]}
    else:
        got = {"dq": fh(dq).bfloat16(), "dk": fh(dk).bfloat16(), "dv": fh(dv).bfloat16()}
    A.check_all(got, vals, bounds, f"fused qpre={qpre:.2f} sqk={with_sqk}")
    if with_sqk:     # a dK left at scale (mutant h) is seen through the epilogue too
        if qpre != 1.0:
            bad = A.emulate_bwd(c, o, lse, mutant="h_dk_scale", raw=True)[1]
            cc["gk"] = bad
            assert A.margin(A.qknorm_bwd_formula(cc, fwd, torch.float32)["dk"].bfloat16(), vals["dk"], bounds["dk"]) >= 2.0


def test_bf16_unit_roundoff():
    """one round to nearest even to bf16 errs by up to U16 = 2^-8 of the value (bottom of a binade), not 2^-9 (top):
    `rel16` is the exact half ulp, between the two"""
    x = torch.tensor([1.0 + 2.0 ** -8, 2.0 - 2.0 ** -8, 1.5 + 2.0 ** -8], dtype=torch.float64)
    err = (x.float().bfloat16().double() - x).abs() / x
    assert err[0] > 2.0 ** -9 and (err <= A.U16).all()
    assert (err <= A.rel16(x) * (1 + 1e-12)).all() and (A.rel16(x) <= A.U16).all() and (A.rel16(x) > 2.0 ** -9).all()
