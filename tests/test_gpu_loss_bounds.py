"""GPU tests, op level: nvit_ce_loss, nvit_ce_loss_soft and nvit_eval_metrics (misc.hip) against the fp64 references
and per-element error bounds of loss_check.py: logits that need the max subtraction, saturated and masked rows, rows of
equal logits, N at the 64- and 256-lane edges, B past the 256 rows of one sweep of the mean, labels outside [0, N)
(2^31 and 2^32 + 1 among them) and NaN logits.  test_loss_check.py shows on the CPU that these bounds pass a correct
fp32 restatement and fail the mutants named there.  Run on the MI355X box: pytest -m gpu.

Largest err/bound seen on the MI355X (observations against the fp64 reference; no bound is set from them):
  nvit_ce_loss        gauss 0.318   shifted 0.316   peaked 0.441   counting 0.019   masked 0.321
  nvit_ce_loss_soft   gauss 0.196   shifted 0.200   peaked 0.441   counting 0.102   masked 0.198
  nvit_eval_metrics   levels 0.047  shifted 0.254   counting 0.057  two accumulating calls 0.075
  (exact, so without a figure: the rows of an out-of-range label, the -inf logits of `masked`, every count and percentage are exact)
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_check as gc
import kohonen_check as kc
import loss_check as lc
from attn_check import Padded, SENTINEL

KEYS = ("rowloss", "loss", "dlogits")


def dev():
    return torch.device("cuda:0")


def run_ce(c):
    """The entry point on NaN-margined inputs and sentinel-margined outputs; returns the three outputs on the CPU."""
    from nvit_amd import ops
    lib = ops._lib.load()
    z = c["z"]
    B, N = z.shape
    zp = Padded((B, N), torch.float32, float("nan"), z.to(dev()))
    out = {"rowloss": Padded((B,), torch.float32, SENTINEL), "loss": Padded((1,), torch.float32, SENTINEL),
           "dlogits": Padded((B, N), torch.float32, SENTINEL)}
    y = c["y"].to(dev())
    if c["y2"] is None:
        ops.check(lib.nvit_ce_loss(zp.ptr(), ops._p(y), out["rowloss"].ptr(), out["loss"].ptr(), out["dlogits"].ptr(),
                                   B, N, ops._s()), "nvit_ce_loss")
    else:
        y2, lam = c["y2"].to(dev()), c["lam"].to(dev())
        ops.check(lib.nvit_ce_loss_soft(zp.ptr(), ops._p(y), ops._p(y2), ops._p(lam), c["eps"], out["rowloss"].ptr(),
                                        out["loss"].ptr(), out["dlogits"].ptr(), B, N, ops._s()), "nvit_ce_loss_soft")
    torch.cuda.synchronize()
    assert zp.margins_intact() and all(o.margins_intact() for o in out.values()), c["name"]
    got = {k: o.t.cpu() for k, o in out.items()}
    got["loss"] = got["loss"][0]
    return got


def hold(c, worst):
    ref = lc.ce_eval(c)
    got = run_ce(c)
    kind = "hard" if c["y2"] is None else "soft"
    fam = c["name"].split()[0]
    m = kc.check_all(got, ref, lc.ce_bounds(c, ref), c["name"], verbose=False)
    worst[(kind, fam)] = max(worst.get((kind, fam), 0.0), m)
    return got


@pytest.mark.parametrize("B,N", lc.CE_SHAPES + [lc.CE_COUNTING_ONLY])
def test_ce_loss_hard_and_soft_within_fp64_bounds(B, N):
    worst = {}
    for fam in lc.families_of(B, N):
        for cfg in lc.HARD_CONFIGS:
            c = lc.hard_case(fam, B, N, cfg, seed=B + N)
            if c is None:
                continue
            got = hold(c, worst)
            oor = (c["y"] < 0) | (c["y"] >= N)
            assert (got["rowloss"][oor] == 0).all(), c["name"]
            if fam == "masked":
                assert (got["dlogits"][c["z"] == lc.NEG_INF] == 0).all()
            if cfg[0] == "in":
                again = run_ce(c)
                assert all(gc.bits_equal(again[k], got[k]) for k in KEYS), f"{c['name']}: two runs differ"
        for cfg in lc.SOFT_CONFIGS:
            c = lc.soft_case(fam, B, N, cfg, seed=B + N)
            if c is not None:
                got = hold(c, worst)
                if fam == "masked":
                    assert (got["dlogits"][c["z"] == lc.NEG_INF] == 0).all()
    for (kind, fam), m in sorted(worst.items()):
        print(f"   ce {kind} {fam} B{B} N{N}: max err/bound {m:.3f}")


def test_ce_loss_every_out_of_range_label_in_one_batch():
    """One row per out-of-range value and one valid row: the six rows have rowloss 0 and a plain softmax / B gradient,
    the loss is the valid row's divided by B = 7; as y of the hard loss and as y, y2 and both of the soft loss."""
    N, B = 65, 7
    z, _ = lc.logits("gauss", B, N, 5)
    y = torch.tensor(lc.out_of_range(N) + [1], dtype=torch.int64)
    inr = torch.full((B,), 1, dtype=torch.int64)
    worst = {}
    got = hold({"z": z, "y": y, "y2": None, "lam": None, "eps": 0.0, "name": "gauss all_out"}, worst)
    assert (got["rowloss"][:6] == 0).all() and got["rowloss"][6] > 0
    sm = torch.softmax(z.double(), dim=1) / B
    assert (got["dlogits"][:6].double() - sm[:6]).abs().max() < 1e-7
    for a, b in ((y, inr), (inr, y), (y, y)):
        for eps in (0.0, 0.1):
            hold({"z": z, "y": a, "y2": b, "lam": torch.full((B,), 0.3), "eps": eps, "name": "gauss all_out_soft"}, worst)


# ------------------------------------------------------------------------------------------------ evaluation metrics
def run_metrics(z, y, acc=None):
    from nvit_amd import ops
    B, N = z.shape
    zp = Padded((B, N), torch.float32, float("nan"), z.to(dev()))
    if acc is None:
        acc = Padded((4,), torch.float32, SENTINEL)
        acc.t.zero_()
    ops.eval_metrics(zp.t, y.to(dev()), acc.t)
    torch.cuda.synchronize()
    assert zp.margins_intact() and acc.margins_intact()
    return acc


@pytest.mark.parametrize("N", lc.EVAL_N)
def test_eval_metrics_loss_bounded_counts_exact(N):
    worst = {}
    for B in lc.EVAL_B:
        for fam in lc.EVAL_FAMILIES:
            z = lc.eval_logits(fam, B, N, seed=3 * B + N)
            for mode, k in (("in", 0), ("out", 0), ("out", 1)):
                y = lc.eval_labels(z, 5, mode, k)
                loss, c1, ck = lc.eval_metrics_eval(z, y)
                acc = run_metrics(z, y).t.cpu()
                label = f"eval {fam} {mode}{k} B{B} N{N}"
                m = kc.check(acc[0], loss, lc.eval_metrics_bounds(z, y), label, verbose=False)
                worst[fam] = max(worst.get(fam, 0.0), m)
                assert acc[1].item() == lc.percent(c1, B).item() and acc[2].item() == lc.percent(ck, B).item(), label
                assert acc[3].item() == 1.0
                if mode == "out" and B == 1:
                    assert acc[0].item() == 0.0 and acc[1].item() == 0.0 and acc[2].item() == 0.0
            assert gc.bits_equal(run_metrics(z, y).t.cpu(), acc), "two runs differ"
    for fam, m in sorted(worst.items()):
        print(f"   eval_metrics {fam} N{N}: max err/bound {m:.3f}")


def test_eval_metrics_two_accumulating_calls():
    (Ba, Na), (Bb, Nb) = (33, 65), (17, 6)
    za, zb = lc.eval_logits("shifted", Ba, Na, 1), lc.eval_logits("levels", Bb, Nb, 2)
    ya, yb = lc.eval_labels(za, 3, "out", 0), lc.eval_labels(zb, 4)
    (la, a1, ak), (lb, b1, bk) = lc.eval_metrics_eval(za, ya), lc.eval_metrics_eval(zb, yb)
    acc = run_metrics(za, ya)
    acc = run_metrics(zb, yb, acc).t.cpu()
    bound = lc.eval_metrics_bounds(za, ya) + lc.eval_metrics_bounds(zb, yb, acc_before=la.item())
    kc.check(acc[0], la + lb, bound, "eval two calls")
    assert acc[1].item() == (lc.percent(a1, Ba) + lc.percent(b1, Bb)).item()
    assert acc[2].item() == (lc.percent(ak, Ba) + lc.percent(bk, Bb)).item()
    assert acc[3].item() == 2.0


@pytest.mark.parametrize("N", [8, 65, 1000])
def test_eval_metrics_nan_logits_rank_as_in_topk(N):
    """One NaN on, before and after the label, and two NaNs: the counts of loss_check.ranks (held to torch.topk on the
    CPU); a row whose label logit is NaN is a hit only when no NaN precedes it; the accumulated loss is NaN."""
    z, y, nn = lc.nan_rows(N, seed=N)
    loss, c1, ck = lc.eval_metrics_eval(z, y)
    assert (c1, ck) == (4, 10) and math.isnan(loss.item())
    acc = run_metrics(z, y).t.cpu()
    assert math.isnan(acc[0].item())
    assert acc[1].item() == lc.percent(c1, 10).item() and acc[2].item() == lc.percent(ck, 10).item()
    for i in range(10):                                  # row by row, so that two errors cannot cancel in the counts
        ok, rank = lc.ranks(z[i:i + 1], y[i:i + 1])
        a = run_metrics(z[i:i + 1], y[i:i + 1]).t.cpu()
        assert a[1].item() == (100.0 if rank[0] < 1 else 0.0) and a[2].item() == (100.0 if rank[0] < 5 else 0.0), i
        if nn[i] <= 1:
            assert (int(a[1].item() == 100.0), int(a[2].item() == 100.0)) == lc.topk_counts(z[i:i + 1], y[i:i + 1]), i
    diverged = torch.full((5, N), float("nan"))          # a diverged model: only the label at class 0 is "first"
    acc = run_metrics(diverged, torch.tensor([0, 1, 4, 5, N - 1])).t.cpu()
    assert acc[1].item() == lc.percent(1, 5).item() and acc[2].item() == lc.percent(3, 5).item()
