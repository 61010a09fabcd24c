"""GPU: nvit_ema_tick / nvit_ema_update op by op, on tables of hand-made tensors (no model).

Row lengths at every edge of the chunking (1, 3, 4, 10, 4096, 4097, chunk + 4, 3 chunks + 1), a view that starts at
element 1 of its buffer (misaligned: the element-wise path), and one row of more chunks than the grid has workgroups
(a second sweep).  Every destination sits between sentinel words that must keep their bits.  The factor the tick stores
is compared bit for bit with the fp64 formula; every updated element with the fp64 update inside the derived bound of
tests/ema_ref.py; copy rows, the skipped step and the refusals bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ema_ref

DEV = "cuda:0"
SENTINEL = 0x7FA5A5A5    # a NaN with a payload: any write over it, and any arithmetic on it, shows
GUARD = 4                # floats ahead of an aligned destination (16 bytes: the view stays aligned)


def _sizes():
    from nvit_amd import ops
    c = ops.EMA_CHUNK
    big = (ops.EMA_MAX_GRID + 1) * c + 4     # more chunks than workgroups: some take a second one
    #       (numel, lead): lead GUARD = aligned, lead 1 = the view starts at element 1 of its buffer
    return [(1, GUARD), (3, GUARD), (4, GUARD), (10, GUARD), (4096, GUARD), (4096, 1), (big, GUARD), (4097, GUARD),
            (c + 4, GUARD), (3 * c + 1, GUARD), (8, 1)]


def _values(n, seed):
    """(e, p) fp32: N(0, 1) mixed with exact zeros, e == p elements and magnitudes 1e-30 and 1e30"""
    rng = np.random.default_rng(seed)
    e, p = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    i = np.arange(n)
    p[i % 7 == 1] = 0.0
    e[i % 7 == 2] = 0.0
    e[i % 7 == 3], p[i % 7 == 3] = 0.0, 0.0
    for m, s in ((i % 11 == 3, np.float32(1e-30)), (i % 11 == 4, np.float32(1e30))):
        e[m] *= s
        p[m] *= s
    e[i % 7 == 0] = p[i % 7 == 0]
    return e, p


class Rows:
    """src and dst tensors of a table on the device, each dst a view into a sentinel-filled buffer"""

    def __init__(self, sizes, seed=0):
        self.sizes = sizes
        self.host = [_values(n, seed + k) for k, (n, _) in enumerate(sizes)]
        self.bufs, self.dst, self.src = [], [], []
        for (n, lead), (e, p) in zip(sizes, self.host):
            buf = torch.empty(lead + n + GUARD, device=DEV, dtype=torch.float32)
            # the sources are views at the same offset, so a misaligned row is misaligned on both sides
            sbuf = torch.zeros(lead + n + GUARD, device=DEV, dtype=torch.float32)
            self.bufs.append(buf)
            self.dst.append(buf[lead:lead + n])
            self.src.append(sbuf[lead:lead + n])
            self.src[-1].copy_(torch.from_numpy(p))
        self.reset()

    def reset(self):
        for buf, d, (e, _) in zip(self.bufs, self.dst, self.host):
            buf.view(torch.int32).fill_(SENTINEL)
            d.copy_(torch.from_numpy(e))

    def pairs(self, copy=False):
        return [(s, d, copy) for s, d in zip(self.src, self.dst)]

    def results(self):
        """[dst as numpy] after checking that every sentinel word and every source kept its bits"""
        out = []
        for (n, lead), buf, s, (_, p) in zip(self.sizes, self.bufs, self.src, self.host):
            words = buf.view(torch.int32).cpu().numpy()
            assert (words[:lead] == SENTINEL).all() and (words[lead + n:] == SENTINEL).all(), (n, lead)
            assert s.cpu().numpy().tobytes() == p.tobytes(), (n, lead)
            out.append(words[lead:lead + n].view(np.float32).copy())
        return out


@pytest.fixture(scope="module")
def rows():
    return Rows(_sizes())


def _state(t=0.0):
    return torch.tensor([float(t), 0.0, 0.0, 0.0], device=DEV)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def test_table_layout_and_flags(rows):
    from nvit_amd import ops
    table, chunks = ops.ema_table(rows.pairs(), torch.device(DEV))
    t = table.cpu()
    assert tuple(t.shape) == (len(rows.sizes), ops.EMA_TABLE_COLS) and t.dtype == torch.int64
    first = 0
    for r, (n, lead), s, d in zip(t.tolist(), rows.sizes, rows.src, rows.dst):
        scalar = bool(n % 4 or lead % 4)
        assert r == [s.data_ptr(), d.data_ptr(), n, first, ops.EMA_FLAG_SCALAR if scalar else 0], (n, lead)
        assert (d.data_ptr() % 16 != 0) == (lead % 4 != 0)
        first += -(-n // ops.EMA_CHUNK)
    assert chunks == first > ops.EMA_MAX_GRID      # a second sweep
    flags = ops.ema_table(rows.pairs(copy=True), torch.device(DEV))[0].cpu()[:, 4].tolist()
    assert all(f & ops.EMA_FLAG_COPY for f in flags)


@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("decay", [0.9998, 0.9])
def test_tick_stores_the_fp64_factor_bit_for_bit(decay, warmup):
    from nvit_amd import ops
    for t in (0, 1, 8, 9, 10, 50000):
        st = _state(t)
        ops.ema_tick(st, decay, warmup)
        got = st.cpu().numpy()
        want = ema_ref.omd_at(t, decay, warmup)
        assert got[1].tobytes() == want.tobytes(), (t, decay, warmup, float(got[1]), float(want))
        assert got[0] == t + 1 and got[2] == 0.0 and got[3] == 0.0, (t, got)
    # consecutive ticks walk the warm-up
    st = _state(0)
    for t in range(12):
        ops.ema_tick(st, decay, warmup)
        assert st[1].cpu().numpy().tobytes() == ema_ref.omd_at(t, decay, warmup).tobytes(), t
    assert st[0].item() == 12.0


@pytest.mark.parametrize("t,decay,warmup", [(0, 0.9998, True), (50000, 0.9998, True), (3, 0.0, False)],
                         ids=["omd0.9", "omd2e-4", "omd1"])
def test_every_element_inside_the_fp64_bound(rows, t, decay, warmup):
    from nvit_amd import ops
    rows.reset()
    table, chunks = ops.ema_table(rows.pairs(), torch.device(DEV))
    st = _state(t)
    ops.ema_tick(st, decay, warmup)
    ops.ema_update(table, chunks, st)
    omd = st[1].cpu().numpy()
    assert omd.tobytes() == ema_ref.omd_at(t, decay, warmup).tobytes() and 0.0 < float(omd) <= 1.0
    worst = 0.0
    for (n, lead), got, (e, p) in zip(rows.sizes, rows.results(), rows.host):
        ref, bound = ema_ref.update64(e, p, omd), ema_ref.update_bound(e, p)
        err = np.abs(got.astype(np.float64) - ref)
        assert np.isfinite(got).all() and (err <= bound).all(), (n, lead, int(np.argmax(err - bound)))
        same = e == p
        assert same.any() or n < 8
        assert got[same].tobytes() == e[same].tobytes(), (n, lead)      # p == e gives e back bit for bit
        nz = bound > 0
        worst = max(worst, float((err[nz] / bound[nz]).max()) if nz.any() else 0.0)
        if float(omd) < 1.0:   # the update did something: elements with p != e moved unless omd (p - e) is below an ulp
            moved = got != e
            assert not moved[same].any() and (moved.any() or n < 8), (n, lead)
    print(f"   ema update t={t} decay={decay}: omd {float(omd):.6g}, max err/bound {worst:.3f}")


def test_copy_rows_are_bit_identical_with_nan_and_inf_payloads(rows):
    from nvit_amd import ops
    rows.reset()
    rng = np.random.default_rng(99)
    raw = []
    for s in rows.src:      # arbitrary words: NaNs of every payload, infinities, denormals
        w = rng.integers(-2 ** 31, 2 ** 31, size=s.numel(), dtype=np.int64).astype(np.int32)
        w[:3] = np.array([0x7F800000, -8388608, 0x7FC00001], dtype=np.int32)[:min(3, w.size)]   # +inf, -inf, a NaN
        raw.append(w)
        s.view(torch.int32).copy_(torch.from_numpy(w))
    try:
        table, chunks = ops.ema_table(rows.pairs(copy=True), torch.device(DEV))
        ops.ema_update(table, chunks)      # no state: the copy rows run
        for (n, lead), buf, w in zip(rows.sizes, rows.bufs, raw):
            words = buf.view(torch.int32).cpu().numpy()
            assert (words[:lead] == SENTINEL).all() and (words[lead + n:] == SENTINEL).all(), (n, lead)
            assert words[lead:lead + n].tobytes() == w.tobytes(), (n, lead)
    finally:
        for s, (_, p) in zip(rows.src, rows.host):
            s.copy_(torch.from_numpy(p))


def test_copy_and_average_rows_share_a_table_and_no_state_means_copies_only(rows):
    from nvit_amd import ops
    rows.reset()
    pairs = [(s, d, k % 2 == 0) for k, (s, d) in enumerate(zip(rows.src, rows.dst))]
    table, chunks = ops.ema_table(pairs, torch.device(DEV))
    ops.ema_update(table, chunks)          # no state: the averaging rows are left alone
    for k, (got, (e, p)) in enumerate(zip(rows.results(), rows.host)):
        assert got.tobytes() == (p if k % 2 == 0 else e).tobytes(), k
    rows.reset()
    st = _state(0)
    ops.ema_tick(st, 0.9998, True)
    ops.ema_update(table, chunks, st)
    omd = st[1].cpu().numpy()
    for k, (got, (e, p)) in enumerate(zip(rows.results(), rows.host)):
        if k % 2 == 0:
            assert got.tobytes() == p.tobytes(), k
        else:
            assert (np.abs(got - ema_ref.update64(e, p, omd)) <= ema_ref.update_bound(e, p)).all(), k
            assert got.tobytes() != e.tobytes() or got.size < 2, k


def test_skipped_step_leaves_every_bit_and_the_count(rows):
    from nvit_amd import ops
    rows.reset()
    table, chunks = ops.ema_table(rows.pairs(), torch.device(DEV))
    st = _state(7)
    st[1] = 0.125      # a stale factor of an earlier update must not be used
    skip = torch.tensor([1.0, 5.0], device=DEV)
    ops.ema_tick(st, 0.9998, True, skip)
    ops.ema_update(table, chunks, st)
    assert st.tolist() == [7.0, 0.0, 0.0, 0.0] and skip.tolist() == [1.0, 5.0]
    for got, (e, _) in zip(rows.results(), rows.host):
        assert got.tobytes() == e.tobytes()
    # the flag down: the bits of the unguarded call
    skip[0] = 0.0
    ops.ema_tick(st, 0.9998, True, skip)
    ops.ema_update(table, chunks, st)
    guarded, gstate = rows.results(), st.tolist()
    rows.reset()
    st2 = _state(7)
    ops.ema_tick(st2, 0.9998, True)
    ops.ema_update(table, chunks, st2)
    assert gstate == st2.tolist() and gstate[0] == 8.0 and gstate[1] > 0.0
    for a, b, (e, _) in zip(guarded, rows.results(), rows.host):
        assert a.tobytes() == b.tobytes()
        assert a.tobytes() != e.tobytes() or a.size < 2


def test_overlapping_and_identical_ranges_are_refused_before_anything_is_written():
    from nvit_amd import ops
    dev = torch.device(DEV)
    buf = torch.arange(64, device=DEV, dtype=torch.float32)
    other = torch.arange(64, 96, device=DEV, dtype=torch.float32)
    keep, keep_other = _bits(buf).clone(), _bits(other).clone()
    bad = {
        "src is dst": [(buf[:16], buf[:16])],
        "dst overlaps its src": [(buf[:16], buf[8:24])],
        "dst overlaps its src by one element": [(buf[:16], buf[15:31])],
        "dst overlaps another row's src": [(buf[:16], other[:16]), (other[8:24], buf[32:48])],
        "two rows share a dst": [(buf[:16], other[:16]), (buf[16:32], other[:16])],
        "two rows' dst overlap": [(buf[:16], other[:16]), (buf[16:32], other[12:28])],
        "a copy row onto itself": [(buf[:16], buf[:16], True)],
    }
    for what, pairs in bad.items():
        with pytest.raises(ValueError):
            ops.ema_table(pairs, dev)
    with pytest.raises(ValueError):
        ops.ema_table([(buf[:16], other[:8])], dev)      # lengths differ
    with pytest.raises(ValueError):
        ops.ema_table([], dev)
    # neighbours that only touch, and one source feeding two destinations, are fine
    table, chunks = ops.ema_table([(buf[:16], buf[16:32], True), (buf[:16], other[:16], True)], dev)
    assert _bits(buf).equal(keep) and _bits(other).equal(keep_other)      # nothing was written by any of the above
    ops.ema_update(table, chunks)
    assert torch.equal(buf[16:32], buf[:16]) and torch.equal(other[:16], buf[:16]) and _bits(buf[32:]).equal(keep[32:])
