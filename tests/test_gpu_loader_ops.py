"""GPU: the two kernels of the device-resident dataset (loader.hip, nvit_amd/data.py).  nvit_loader_draw against the numpy
twin tests/loader_ref.py, bit for bit, at epoch borders and with the counter preset beyond 32 bits; nvit_loader_gather
against `images[idx]` / `labels[idx]`, bit for bit, on both of its paths (16-byte vectors, single bytes), on an unaligned
dataset tensor, next to a guard region, and at a byte offset beyond 2^32."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import loader_ref as R
from nvit_amd import DeviceDataset


def dev():
    return torch.device("cuda:0")


def labelled(N):
    """A dataset of one-byte images whose only use is its size: the draw reads no image."""
    return DeviceDataset(torch.zeros(N, 1, 1, 1, dtype=torch.uint8, device=dev()), torch.arange(N, device=dev()))


# ------------------------------------------------------------------------------------------------ draw
@pytest.mark.parametrize("N,B,world,repeats", [(1, 1, 1, 1), (17, 8, 1, 1), (37, 8, 2, 1), (4097, 64, 1, 3), (50000, 512, 1, 1)],
                         ids=lambda v: str(v))
def test_draw_equals_the_twin_bit_for_bit(N, B, world, repeats):
    ds = labelled(N)
    seed = 2 ** 40 + 17
    for rank in range(world):
        ld = ds.loader(B, seed=seed, world_size=world, rank=rank, repeats=repeats)
        S = ld.steps_per_epoch
        assert S == R.steps_per_epoch(N, B, world, repeats) and ld.record.tolist() == [0, 0]
        # the last step of an epoch and the first of the next; a counter beyond 2^31; an epoch beyond 2^32
        for s0 in (0, S - 1, 3 * S - 1, 2 ** 31 + 3, (2 ** 32 + 5) * S + S - 1):
            ld.load_state_dict({**ld.state_dict(), "step": s0})
            for s in (s0, s0 + 1):
                idx = ld.draw()
                want = R.draw(seed, s, N, B, world, rank, repeats)
                assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), want), (rank, s)
                assert ld.step == s + 1 and ld.record.tolist() == list(divmod(s, S)) and ld.epoch == (s + 1) // S
        plain = ds.loader(B, shuffle=False, seed=seed, world_size=world, rank=rank, repeats=repeats)
        plain.load_state_dict({**plain.state_dict(), "step": S - 1})
        for s in (S - 1, S):
            assert np.array_equal(plain.draw().cpu().numpy(), R.draw(seed, s, N, B, world, rank, repeats, shuffle=False))
    if world == 2:   # the two ranks' rows are the one-rank loader's global batch
        whole = ds.loader(B * world, seed=seed, repeats=repeats).draw().cpu().numpy()
        parts = [ds.loader(B, seed=seed, world_size=2, rank=r, repeats=repeats).draw().cpu().numpy() for r in (0, 1)]
        assert np.array_equal(whole, np.concatenate(parts))


def test_draw_covers_an_epoch_once_and_another_seed_draws_another_order():
    N, B = 4097, 64
    ds = labelled(N)
    ld, other = ds.loader(B, seed=1), ds.loader(B, seed=2)
    S = ld.steps_per_epoch
    epochs = [torch.cat([ld.draw() for _ in range(S)]).cpu().numpy() for _ in range(2)]
    for e in epochs:
        assert len(np.unique(e)) == S * B == 4096 and e.min() >= 0 and e.max() < N
    assert (epochs[0] == epochs[1]).mean() < 0.02
    assert (torch.cat([other.draw() for _ in range(S)]).cpu().numpy() == epochs[0]).mean() < 0.02
    assert ld.step == 2 * S and ld.epoch == 2


# ------------------------------------------------------------------------------------------------ gather
GUARD = 4096


def gather_raw(images, labels, idx):
    """nvit_loader_gather into a buffer with a guard region behind the batch and one behind the labels."""
    from nvit_amd import ops
    from nvit_amd._lib import call
    N, row = images.shape[0], images[0].numel()
    B = idx.shape[0]
    out = torch.full((B * row + GUARD,), 0xA5, dtype=torch.uint8, device=dev())
    y = torch.full((B + 8,), -7, dtype=torch.int64, device=dev())
    call("nvit_loader_gather", images, labels, idx, out, y, N, row, B, ops._s())
    assert (out[B * row:] == 0xA5).all() and (y[B:] == -7).all(), "the guard regions were written"
    return out[:B * row].view(B, *images.shape[1:]), y[:B]


@pytest.mark.parametrize("shape", [(5, 7, 1), (32, 32, 3), (24, 40, 3), (33, 33, 3), (64, 64, 3)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
def test_gather_equals_indexing_bit_for_bit(shape, offset):
    """Rows of 35, 3072, 2880, 3267 and 12288 bytes (the last: three chunks per row); offset 1: the dataset tensor is a view
    one byte into its allocation, so its base is unaligned and every row takes the byte path."""
    N, row = 61, int(np.prod(shape))
    g = np.random.default_rng(row + offset)
    store = torch.from_numpy(g.integers(0, 256, (N * row + 16,), dtype=np.uint8)).to(dev())
    images = store[offset:offset + N * row].view(N, *shape)
    labels = torch.from_numpy(g.integers(0, 1000, (N,))).to(dev())
    assert images.data_ptr() % 16 == offset and images.is_contiguous()
    ds = DeviceDataset(images, labels)
    for idx in ([0, N - 1], [N - 1, 0, 0, 7, 7, 7, N - 1, 30, 0], list(g.integers(0, N, 130)), [N - 1]):
        idx = torch.tensor(idx, dtype=torch.int64, device=dev())
        got, y = gather_raw(images, labels, idx)
        assert torch.equal(got, images[idx]) and torch.equal(y, labels[idx]), (shape, offset, idx.tolist()[:4])
        out, y2 = ds.take(idx)           # the product's call, into tensors of its own
        assert out.shape == (idx.shape[0], *shape) and torch.equal(out, images[idx]) and torch.equal(y2, labels[idx])
    assert torch.equal(store.cpu(), torch.from_numpy(np.random.default_rng(row + offset).integers(0, 256, (N * row + 16,), dtype=np.uint8)))


def test_gather_into_an_unaligned_batch_takes_the_byte_path():
    N, shape = 9, (8, 8, 1)
    g = np.random.default_rng(3)
    images = torch.from_numpy(g.integers(0, 256, (N, *shape), dtype=np.uint8)).to(dev())
    labels = torch.arange(N, device=dev())
    idx = torch.tensor([8, 0, 3, 3], dtype=torch.int64, device=dev())
    from nvit_amd import ops
    from nvit_amd._lib import call
    buf = torch.full((4 * 64 + 32,), 0x5A, dtype=torch.uint8, device=dev())
    y = torch.empty(4, dtype=torch.int64, device=dev())
    call("nvit_loader_gather", images, labels, idx, buf[3:], y, N, 64, 4, ops._s())
    assert torch.equal(buf[3:3 + 256].view(4, *shape), images[idx]) and (buf[:3] == 0x5A).all() and (buf[259:] == 0x5A).all()


def test_an_index_outside_the_dataset_reads_nothing():
    images = torch.full((4, 4, 4, 1), 9, dtype=torch.uint8, device=dev())
    labels = torch.tensor([5, 6, 7, 8], device=dev())
    out, y = DeviceDataset(images, labels).take(torch.tensor([3, 4, -1, 0], dtype=torch.int64, device=dev()))
    assert out[:, 0, 0, 0].tolist() == [9, 0, 0, 9] and (out[1:3] == 0).all() and y.tolist() == [8, 0, 0, 5]
    ds = DeviceDataset(images, labels)
    ok = torch.tensor([1, 2], dtype=torch.int64, device=dev())
    for bad, exc in ((ok.int(), ValueError), (ok[None], ValueError), (ok[:0], ValueError), ([1, 2], ValueError),
                     (ok.cpu(), RuntimeError)):      # anything but a device int64 [B] is refused before the launch
        with pytest.raises(exc):
            ds.take(bad)
        with pytest.raises(exc):
            ds.loader(2).gather(bad)


def test_gather_beyond_a_byte_offset_of_two_to_the_32():
    """N = 1400 images of 1024x1024x3: 4.4 GB, so the rows from 1366 on start beyond 2^32 bytes.  Only the rows that are
    read are ever written."""
    N, shape = 1400, (1024, 1024, 3)
    row = int(np.prod(shape))
    assert 1365 * row < 2 ** 32 < 1366 * row
    images = torch.empty((N, *shape), dtype=torch.uint8, device=dev())
    labels = torch.arange(N, device=dev()) * 3
    picks = [1399, 0, 1366, 1365, 1399]
    g = torch.Generator(device=dev()).manual_seed(1)
    for n in set(picks):
        images[n] = torch.randint(0, 256, shape, dtype=torch.uint8, device=dev(), generator=g)
    idx = torch.tensor(picks, dtype=torch.int64, device=dev())
    out, y = DeviceDataset(images, labels).take(idx)
    for b, n in enumerate(picks):
        assert torch.equal(out[b], images[n]), n
    assert y.tolist() == [3 * n for n in picks] and not torch.equal(out[0], out[2])


def test_loader_call_is_draw_then_gather():
    g = np.random.default_rng(8)
    N = 100
    images = torch.from_numpy(g.integers(0, 256, (N, 8, 8, 3), dtype=np.uint8)).to(dev())
    labels = torch.from_numpy(g.integers(0, 10, (N,))).to(dev())
    ld = DeviceDataset(images, labels).loader(16, seed=4, repeats=3)
    for s in range(3):
        u8, y = ld()
        idx = torch.from_numpy(R.draw(4, s, N, 16, repeats=3)).to(dev())
        assert torch.equal(u8, images[idx]) and torch.equal(y, labels[idx]) and ld.step == s + 1
