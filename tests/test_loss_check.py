"""The oracles of loss_check.py have teeth (CPU only, no GPU): the fp32 restatement of the cross-entropy, soft-target
cross-entropy and evaluation-metric kernels stays inside the bounds at every shape, family and label set of the GPU
tests, the reference has the closed forms its families are built for, and every mutant - a way the kernel can go wrong
without crashing - falls outside a bound on a listed case (printed)."""
import math

import pytest
import torch

import kohonen_check as kc
import loss_check as lc

F32, F64 = torch.float32, torch.float64
KEYS = ("rowloss", "loss", "dlogits")


def cases_of(B, N):
    for fam in lc.families_of(B, N):
        for cfg in lc.HARD_CONFIGS:
            c = lc.hard_case(fam, B, N, cfg, seed=B + N)
            if c is not None:
                yield c
        for cfg in lc.SOFT_CONFIGS:
            c = lc.soft_case(fam, B, N, cfg, seed=B + N)
            if c is not None:
                yield c


def inside(c, got, ref=None, verbose=False):
    ref = lc.ce_eval(c) if ref is None else ref
    return kc.check_all(got, ref, lc.ce_bounds(c, ref), c["name"], verbose)


@pytest.mark.parametrize("B,N", lc.CE_SHAPES + [lc.CE_COUNTING_ONLY])
def test_ce_fp32_restatement_inside_the_bounds(B, N):
    worst = 0.0
    for c in cases_of(B, N):
        ref = lc.ce_eval(c)
        assert all(torch.isfinite(ref[k]).all() for k in KEYS), c["name"]
        worst = max(worst, inside(c, lc.ce_eval(c, F32), ref))
    print(f"   ce B{B} N{N}: largest err/bound of the fp32 restatement {worst:.3f}")


def test_shapes_cover_the_edges_of_the_issue():
    assert {N for B, N in lc.CE_SHAPES if B == 3} == set(lc.CE_N)
    for N in (65, 257):
        assert {B for B, n in lc.CE_SHAPES if n == N} == set(lc.CE_B)
    assert len(set(lc.CE_SHAPES)) == len(lc.CE_SHAPES)
    # every out-of-range value is a label of some row, as y and as y2; at B = 3 the two large ones are
    for N in (65, 257):
        for B in (257, 1000):
            y = lc.labels(B, N, 1, "out", 0).tolist() + lc.labels(B, N, 1, "out", 1).tolist()
            assert set(lc.out_of_range(N)) <= set(y) and any(0 <= v < N for v in y)
    seen = set(lc.labels(3, 65, 1, "out", 0).tolist()) | set(lc.labels(3, 65, 1, "out", 1).tolist())
    assert {2 ** 32 + 1, 2 ** 31, -1, 65} <= seen
    assert lc.narrow32(torch.tensor([2 ** 32 + 1, 2 ** 31, -1, 7])).tolist() == [1, -2 ** 31, -1, 7]


def test_reference_closed_forms():
    """counting: softmax = 1/N and rowloss = ln N whatever the row's constant; out-of-range rows: rowloss 0, a plain
    softmax row, and the loss still divided by B; masked: exactly 0 with a bound of exactly 0 at a -inf logit."""
    for B, N in [(3, 65), (257, 257), lc.CE_COUNTING_ONLY]:
        c = lc.hard_case("counting", B, N, lc.HARD_CONFIGS[0], 1)
        ref = lc.ce_eval(c)
        assert (ref["rowloss"] - math.log(N)).abs().max() < 1e-12 and abs(ref["loss"].item() - math.log(N)) < 1e-12
        sm = ref["dlogits"] * B + torch.nn.functional.one_hot(c["y"], N)
        assert (sm - 1.0 / N).abs().max() < 1e-15
    c = lc.hard_case("counting", 3, 65, lc.HARD_CONFIGS[1], 1)
    assert c["y"].tolist()[0] == 2 ** 32 + 1 and c["y"].tolist()[2] == 2 ** 31
    ref = lc.ce_eval(c)
    assert ref["rowloss"].tolist()[0] == 0.0 and ref["rowloss"].tolist()[2] == 0.0
    assert abs(ref["loss"].item() - math.log(65) / 3) < 1e-12
    assert (ref["dlogits"][0] * 3 - 1.0 / 65).abs().max() < 1e-15
    c = lc.hard_case("masked", 257, 257, lc.HARD_CONFIGS[0], 1)
    ref, masked = lc.ce_eval(c), c["z"] == lc.NEG_INF
    assert 0.05 < masked.double().mean() < 0.15 and not masked[torch.arange(257), c["y"]].any()
    assert (ref["dlogits"][masked] == 0).all() and (lc.ce_bounds(c, ref)["dlogits"][masked] == 0).all()
    assert (lc.ce_eval(c, F32)["dlogits"][masked] == 0).all()
    # against torch where the two definitions agree: labels in range, the mean over all rows
    c = lc.soft_case("gauss", 33, 100, lc.SOFT_CONFIGS[0], 2)
    ref = lc.ce_eval(c)
    eps = torch.tensor(c["eps"], dtype=F32).double()
    oh = torch.nn.functional.one_hot
    lam = c["lam"].double()[:, None]
    t = (1 - eps) * (lam * oh(c["y"], 100) + (1 - lam) * oh(c["y2"], 100)) + eps / 100
    zr = c["z"].double().requires_grad_(True)
    want = torch.nn.functional.cross_entropy(zr, t)
    (g,) = torch.autograd.grad(want, zr)
    assert abs(want.item() - ref["loss"].item()) < 1e-12 and (g - ref["dlogits"]).abs().max() < 1e-15


# where each mutant is shown: (B, N, family, "hard" | "soft", config index); more than one for the mutants whose listed
# edge is a set of sizes
CE_KILLS = {
    "no_max": [(3, 65, "shifted", "hard", 0), (3, 65, "shifted", "soft", 0)],
    "max_first256": [(257, 257, "peaked", "hard", 0), (3, 1000, "peaked", "soft", 0)],
    "drop_last_col": [(3, 65, "counting", "hard", 0), (3, 257, "counting", "hard", 0), (3, 1023, "counting", "soft", 0)],
    "rowloss_first256": [(257, 65, "counting", "hard", 0), (1000, 257, "gauss", "soft", 0)],
    "div_valid": [(3, 65, "gauss", "hard", 1), (1, 65, "gauss", "hard", 2)],
    "narrow32": [(3, 65, "gauss", "hard", 1), (3, 3, "gauss", "soft", 3), (257, 257, "gauss", "soft", 3)],
    "smooth_nm1": [(3, 65, "gauss", "soft", 0), (3, 3, "gauss", "soft", 2)],
    "lam_swapped": [(3, 65, "gauss", "soft", 0), (257, 257, "gauss", "soft", 5)],
}


def test_every_mutant_is_listed():
    assert set(CE_KILLS) == set(lc.CE_MUTANTS)
    for where in CE_KILLS.values():
        for B, N, fam, kind, i in where:
            assert (B, N) in lc.CE_SHAPES and fam in lc.CE_FAMILIES


@pytest.mark.parametrize("mutant", lc.CE_MUTANTS)
def test_ce_mutant_falls_outside_a_bound(mutant):
    for B, N, fam, kind, i in CE_KILLS[mutant]:
        c = (lc.hard_case(fam, B, N, lc.HARD_CONFIGS[i], B + N) if kind == "hard"
             else lc.soft_case(fam, B, N, lc.SOFT_CONFIGS[i], B + N))
        inside(c, lc.ce_eval(c, F32))
        with pytest.raises(AssertionError):
            inside(c, lc.ce_eval(c, F32, mutant))
        print(f"   {mutant}: outside the bounds on B{B} N{N} {kind} {c['name']}")


# ------------------------------------------------------------------------------------------------ evaluation metrics
def eval_cases(B, N):
    for fam in lc.EVAL_FAMILIES:
        z = lc.eval_logits(fam, B, N, seed=3 * B + N)
        yield fam, "in", z, lc.eval_labels(z, 5)
        for k in (0, 1):
            yield fam, f"out{k}", z, lc.eval_labels(z, 5, "out", k)


@pytest.mark.parametrize("N", lc.EVAL_N)
def test_eval_metrics_fp32_restatement_and_counts(N):
    worst = 0.0
    for B in lc.EVAL_B:
        for fam, mode, z, y in eval_cases(B, N):
            loss, c1, ck = lc.eval_metrics_eval(z, y)
            got, g1, gk = lc.eval_metrics_eval(z, y, F32)
            assert (g1, gk) == (c1, ck)
            worst = max(worst, kc.check(got, loss, lc.eval_metrics_bounds(z, y), f"eval {fam} {mode}", verbose=False))
            ok = (y >= 0) & (y < N)
            if fam == "counting":      # all logits equal: a top-1 hit iff the label is class 0, a top-k hit iff below min(5, N)
                assert c1 == int((ok & (y == 0)).sum()) and ck == int((ok & (y < min(5, N))).sum())
            elif mode == "in":
                s = z.sort(dim=1).values
                if bool((s[:, 1:] != s[:, :-1]).all()):
                    assert (c1, ck) == lc.topk_counts(z, y), (fam, B, N)
                if fam == "levels" and B >= 5 and N >= 6:
                    assert 0 < c1 < ck < B                      # hits, top-k-only hits and misses all occur
            else:
                keep = ok.nonzero()[:, 0]
                assert (c1, ck) == (lc.eval_metrics_eval(z[keep], y[keep])[1:] if keep.numel() else (0, 0))
                if B == 1:
                    assert loss.item() == 0.0 and (c1, ck) == (0, 0)
    print(f"   eval N{N}: largest err/bound of the fp32 restatement {worst:.3f}")


def test_percent_is_the_fp32_formula():
    for count, B in [(1, 3), (2, 3), (999, 1000), (17, 17), (0, 5)]:
        want = torch.tensor(100.0, dtype=F32) * torch.tensor(float(count), dtype=F32) / torch.tensor(float(B), dtype=F32)
        assert lc.percent(count, B).dtype == F32 and lc.percent(count, B).item() == want.item()


EVAL_KILLS = {"tie_high": [(17, 6, "counting", "in", 0), (33, 65, "counting", "in", 0)],
              "rank_le_maxk": [(17, 6, "levels", "in", 0), (1000, 4099, "shifted", "in", 0)],
              "narrow32": [(17, 6, "levels", "out", 0), (1, 2, "levels", "out", 0)]}


@pytest.mark.parametrize("mutant", lc.EVAL_MUTANTS)
def test_eval_mutant_changes_a_count(mutant):
    for B, N, fam, mode, k in EVAL_KILLS[mutant]:
        assert B in lc.EVAL_B and N in lc.EVAL_N
        z = lc.eval_logits(fam, B, N, seed=3 * B + N)
        y = lc.eval_labels(z, 5, mode, k)
        assert lc.eval_metrics_eval(z, y)[1:] != lc.eval_metrics_eval(z, y, mutant=mutant)[1:]
        print(f"   {mutant}: a wrong count on B{B} N{N} {fam} {mode}")


@pytest.mark.parametrize("N", [8, 65, 1000])
def test_nan_rank_rule_is_topk(N):
    """Row by row against torch.topk where it is defined by the reference (at most one NaN), and the stated rule for
    two: a NaN that is not the label's outranks the label; a NaN label logit is a hit only when no NaN precedes it."""
    z, y, nn = lc.nan_rows(N, seed=N)
    assert nn.tolist() == [1, 1, 1, 1, 1, 1, 2, 2, 0, 0]
    ok, rank = lc.ranks(z, y)
    assert ok.all()
    #          on the label   before: pushed down   after: pushed down   two NaNs   none
    assert rank.tolist() == [0, 0, 1, 4, 1, 4, 1, 0, 0, 3]
    for i in range(10):
        if nn[i] <= 1:
            c1, ck = lc.topk_counts(z[i:i + 1], y[i:i + 1])
            assert (c1, ck) == (int(rank[i] < 1), int(rank[i] < 5)), i
    loss, c1, ck = lc.eval_metrics_eval(z, y)
    assert math.isnan(loss.item()) and (c1, ck) == (4, 10)
    # the rule before the fix (v > ly is false for every NaN): all three NaN-label rows and nothing else changes
    old = ((z > z[torch.arange(10), y][:, None]) | ((z == z[torch.arange(10), y][:, None])
                                                     & (torch.arange(N)[None, :] < y[:, None]))).sum(dim=1)
    assert old.tolist() == [0, 0, 0, 3, 0, 3, 0, 0, 0, 3]
