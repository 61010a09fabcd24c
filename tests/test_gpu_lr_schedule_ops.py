"""GPU tests, op level, of nvit_lr_schedule: synthetic optimizer tables of 1, 7 and 300 rows (300 is more than one pass
of the launch's one workgroup) with random int64 bit patterns in every word the kernel must leave alone, mixed lr_scale
(1, 0.75^k, 0), and the step counter preset to every segment edge.  Per call: the counter is s + 1; the fp64 `last_lr` and
every row's fp32 lr equal the twin (lr_schedule_ref.py) bit for bit wherever no cosine enters; in the cosine segment, where
the device's fp64 cos may differ from the host's in the last place, the derived bound |lr_row - L * scale| <= 2^-24 |L *
scale| + 2^-40 lr; the weight-decay halves and all other table words are bit-identical to what was put in.  One more run
presets the counter to 2^31 + 3 with D = 2^31 + 10: an `int` counter or parameter fails it.  Run on the MI355X box:
pytest -m gpu."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lr_schedule_ref as lr_ref

LR, MIN_LR, W, D = 1e-3, 1e-5, 5, 20
COUNTERS = [0, W - 1, W, W + 1, (W + D) // 2, D - 1, D, D + 1, D + 1000]


def _consts():
    from nvit_amd import _lib
    return _lib.const("OPT_TABLE_COLS"), _lib.const("LR_SCHEDULE_THREADS")


def _table(n, seed):
    cols, _ = _consts()
    rng = np.random.default_rng(seed)
    t = torch.from_numpy(rng.integers(-2 ** 63, 2 ** 63 - 1, (n, cols), dtype=np.int64, endpoint=True))
    k = torch.arange(n)
    scale = torch.where(k % 3 == 0, torch.ones(n, dtype=torch.float64),
                        torch.where(k % 3 == 1, 0.75 ** (k // 3 % 14).double(), torch.zeros(n, dtype=torch.float64)))
    if n >= 3:
        assert (scale == 0).any() and (scale == 1).any() and ((scale > 0) & (scale < 1)).any()
    return t, scale.float()


def _run(kind, s, n, seed, lr=LR, min_lr=MIN_LR, w=W, d=D, warmup_init=0.0):
    """One launch on a fresh table; checks everything a call promises and returns the device's fp64 L."""
    from nvit_amd import ops
    from nvit_amd.schedule import KINDS
    host, scale = _table(n, seed)
    table, scale_dev, sc = host.cuda(), scale.cuda(), scale.numpy()
    step = torch.tensor([s], dtype=torch.int64).cuda()
    last = torch.full((1,), -1.0, dtype=torch.float32).cuda()
    last64 = torch.full((1,), -1.0, dtype=torch.float64).cuda()
    ops.lr_schedule(table, n, scale_dev, step, KINDS[kind], lr, min_lr, warmup_init, w, d, last, last64)
    assert int(step.item()) == s + 1
    got = table.cpu()
    # every word but the low half of the last column is what was put in
    assert torch.equal(got[:, :-1], host[:, :-1])
    assert torch.equal(got[:, -1] >> 32, host[:, -1] >> 32)
    rows = (got[:, -1] & 0xFFFFFFFF).numpy().astype(np.uint32).view(np.float32)
    L = lr_ref.closed_form(kind, s, lr, min_lr, w, d, warmup_init)
    Ldev = float(last64.item())
    assert last.cpu().numpy()[0] == np.float32(Ldev)
    if lr_ref.in_cosine_segment(kind, s, w, d):
        assert abs(Ldev - L) <= 2.0 ** -40 * lr, (kind, s, Ldev, L)
        for i in range(n):
            assert abs(float(rows[i]) - L * float(sc[i])) <= lr_ref.row_bound(L, sc[i], lr), (kind, s, i, rows[i])
            assert rows[i] == lr_ref.row_lr(Ldev, sc[i])          # and the row is the rounding of the device's own L
    else:
        assert lr_ref.f64_bits(Ldev) == lr_ref.f64_bits(L), (kind, s, Ldev, L)
        want = np.array([lr_ref.row_lr(L, sc[i]) for i in range(n)], dtype=np.float32)
        assert np.array_equal(rows.view(np.uint32), want.view(np.uint32)), (kind, s)
    assert (rows[sc == 0] == 0).all()
    return Ldev


@pytest.mark.parametrize("n", [1, 7, 300])
@pytest.mark.parametrize("kind", ["cosine", "linear", "constant"])
def test_every_segment_edge(kind, n):
    assert 300 > _consts()[1]                                       # more rows than the workgroup has threads
    seen = [_run(kind, s, n, seed=100 * n + s) for s in COUNTERS]
    assert seen[0] == 0.0 and seen[1] == LR * (W - 1) / W
    if kind == "constant":
        assert seen[2:] == [LR] * 7
    else:
        assert abs(seen[2] - LR) <= 2.0 ** -40 * LR and abs(seen[6] - MIN_LR) <= 2.0 ** -40 * LR
        assert seen[7] == seen[8] == MIN_LR
        assert LR > seen[3] > seen[4] > seen[5] > MIN_LR


@pytest.mark.parametrize("kind", ["cosine", "linear", "constant"])
def test_warmup_from_a_rate_above_zero_and_no_warmup(kind):
    for s in (0, 1, W - 1, W):
        _run(kind, s, 7, seed=s, warmup_init=1e-6)
    for s in (0, 1, D, D + 1):
        _run(kind, s, 7, seed=50 + s, w=0)


@pytest.mark.parametrize("kind", ["cosine", "linear"])
def test_counter_and_parameters_are_64_bit(kind):
    """s = 2^31 + 3 with D = 2^31 + 10: a counter or a parameter held in an int would land in the warm-up or beyond D."""
    big_d = 2 ** 31 + 10
    got = _run(kind, 2 ** 31 + 3, 300, seed=9, d=big_d)
    assert MIN_LR <= got < MIN_LR + 1e-8                           # seven steps short of D
    assert _run(kind, big_d + 1, 7, seed=10, d=big_d) == MIN_LR
    assert _run(kind, 2 ** 31 + 4, 7, seed=12, w=2 ** 31 + 5, d=2 ** 32) == LR * (2 ** 31 + 4) / (2 ** 31 + 5)
    assert _run("constant", 2 ** 40, 7, seed=11, w=2 ** 31 + 5, d=0) == LR


def test_no_table_only_steps_the_counter():
    from nvit_amd import LRSchedule
    sched = LRSchedule.from_reference(LR, MIN_LR, W, D).to("cuda:0")
    seen = []
    for s in range(D + 3):
        sched.apply()
        seen.append(float(sched.last_lr64.item()))
    assert sched.step == D + 3
    for s, v in enumerate(seen):
        want = sched.lr_at(s)
        assert abs(v - want) <= 2.0 ** -40 * LR and (W <= s <= D or v == want), (s, v, want)
    state = sched.state_dict()
    sched.load_state_dict(dict(state, step=W))              # in place: the same device counter
    sched.apply()
    assert sched.step == W + 1 and float(sched.last_lr.item()) == np.float32(LR)


def test_bad_arguments_are_refused_before_the_launch():
    from nvit_amd import ops
    from nvit_amd.schedule import KINDS
    host, scale = _table(7, 1)
    table, scale = host.cuda(), scale.cuda()
    step = torch.zeros(1, dtype=torch.int64).cuda()
    last, last64 = torch.zeros(1).cuda(), torch.zeros(1, dtype=torch.float64).cuda()
    for kind, w, d, lr in ((7, W, D, LR), (KINDS["cosine"], W, W, LR), (KINDS["linear"], -1, D, LR),
                           (KINDS["cosine"], W, D, -1.0), (KINDS["cosine"], W, D, float("inf"))):
        with pytest.raises(RuntimeError):
            ops.lr_schedule(table, 7, scale, step, kind, lr, MIN_LR, 0.0, w, d, last, last64)
    with pytest.raises(ValueError):
        ops.lr_schedule(table, 7, scale.double(), step, KINDS["cosine"], LR, MIN_LR, 0.0, W, D, last, last64)
    with pytest.raises(ValueError):
        ops.lr_schedule(table, 8, scale, step, KINDS["cosine"], LR, MIN_LR, 0.0, W, D, last, last64)
    assert int(step.item()) == 0 and torch.equal(table.cpu(), host)
