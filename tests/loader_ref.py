"""Oracle of the device-resident dataset's draw (a plain helper module: test_loader_api.py uses it on the CPU,
test_gpu_loader_ops.py and test_gpu_loader.py against the HIP kernels).  It is the definition ("The
device-resident dataset"); nvit_loader_draw (loader.hip) must equal it bit for bit.  Integer arithmetic only.

* `perm`: the stateless bijection of [0, N) per (seed, epoch): a 4-round balanced Feistel network on w bits (w the smallest
  even number of bits that holds N - 1, at least 2) whose round function is a Philox4x32-10 word, cycle-walked.
* `schedule` / `draw`: which image sits in row i of rank r at step s.
"""
from __future__ import annotations

import numpy as np

from mix_ref import M32, philox_vec

DOMAIN = 0x4C4F4144   # xor-ed into the key's high word
ROUNDS = 4


def width(N: int) -> int:
    """The smallest even number of bits that holds N - 1, at least 2."""
    w = max(2, (N - 1).bit_length())
    return w + (w & 1)


def feistel(x: np.ndarray, half: int, seed: int, epoch: int) -> np.ndarray:
    """One pass of the network over uint64 values below 4 ** half."""
    mask = np.uint64((1 << half) - 1)
    L, R = x >> np.uint64(half), x & mask
    n = np.ones(x.shape, dtype=np.uint64)
    for j in range(ROUNDS):
        v0 = philox_vec(R, n * np.uint64(j), n * np.uint64(epoch & 0xFFFFFFFF), n * np.uint64((epoch >> 32) & 0xFFFFFFFF),
                        seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ DOMAIN)[0]
        L, R = R, L ^ (v0 & mask)
    return (L << np.uint64(half)) | R


def perm(x, N: int, seed: int, epoch: int, return_walk: bool = False):
    """perm_{seed,epoch}(x) for an array of values in [0, N): the network, re-applied while the value is >= N.  With
    return_walk also how often it was applied per element."""
    x = np.asarray(x, dtype=np.uint64).copy()
    assert N >= 1 and (x.size == 0 or int(x.max()) < N)
    half = width(N) // 2
    walk = np.zeros(x.shape, dtype=np.int64)
    todo = np.ones(x.shape, dtype=bool)
    while todo.any():
        x[todo] = feistel(x[todo], half, seed, epoch)
        walk[todo] += 1
        todo &= x >= np.uint64(N)
    return (x.astype(np.int64), walk) if return_walk else x.astype(np.int64)


def steps_per_epoch(N: int, B: int, world_size: int = 1, repeats: int = 1) -> int:
    return (N * repeats) // (B * world_size)


def schedule(step: int, N: int, B: int, world_size: int = 1, rank: int = 0, repeats: int = 1):
    """(epoch, step in the epoch, int64 [B] positions // repeats) of rank `rank` at step `step`."""
    G = B * world_size
    S = steps_per_epoch(N, B, world_size, repeats)
    assert S >= 1
    epoch, t = divmod(step, S)
    q = t * G + rank * B + np.arange(B, dtype=np.int64)
    return epoch, t, q // repeats


def draw(seed: int, step: int, N: int, B: int, world_size: int = 1, rank: int = 0, repeats: int = 1,
         shuffle: bool = True) -> np.ndarray:
    """int64 [B]: what nvit_loader_draw writes into idx."""
    epoch, _, p = schedule(step, N, B, world_size, rank, repeats)
    return perm(p, N, seed, epoch) if shuffle else p
