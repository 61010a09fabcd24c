"""The zero-padded-head row kernels at the ViT-H shape (M = 64 x 784 = 50 176 rows, C = 1280 = 16 heads of 80, bf16 mode)
next to the same kernels on compact heads (16 heads of 32, 64 and 128), in one process: HIP-event times and algorithmic
TB/s (the bytes the operation needs: the real columns read, every stored column written, pads included).
python tools/heads_pad_bench.py     (A/B against another build of the library: NVIT_LIB, as tools/rowops_ab.sh does)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from nvit_amd import ops
from nvit_amd._lib import BF16, BF16_F32IN

dev = torch.device("cuda:0")
B, T, H = 64, 784, 16
M = B * T
DP = ops.PAD_HEAD_DIM
g = torch.Generator(device=dev).manual_seed(0)
rn = lambda *s: torch.randn(*s, generator=g, device=dev)


def t_of(fn, n=10):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def report(name, fn, nbytes):
    us = min(t_of(fn) for _ in range(3))
    print(f"  {name}: {us:7.1f} us  {nbytes / us / 1e6:6.2f} TB/s ({nbytes / 1e6:.0f} MB)", flush=True)


def padded(d):
    C = H * d
    qkv = rn(M, 3 * C)
    sqk = torch.full((C,), 1 / 32, device=dev)
    out = ops.heads_pad_fwd(BF16_F32IN, qkv, 3 * C, qkv[:, C:], 3 * C, qkv[:, 2 * C:], 3 * C, sqk, 32.0, B, T, H, d)
    qh, kh, vh, rq, rk, _ = out
    gh = [rn(B, H, T, DP).bfloat16() for _ in range(3)]
    dqkv = torch.empty((M, 3 * C), device=dev, dtype=torch.bfloat16)
    o_p = rn(M, H * DP).bfloat16()
    o = ops.unpad_cols(o_p, M, H, d)
    small = 2 * M * H * 4   # rq, rk
    print(f"padded heads, d = {d} (C = {C}) on {DP}-wide head tensors, M = {M}:")
    report("heads_pad_fwd (normalise) ", lambda: ops.heads_pad_fwd(BF16_F32IN, qkv, 3 * C, qkv[:, C:], 3 * C, qkv[:, 2 * C:],
                                                                   3 * C, sqk, 32.0, B, T, H, d, out=out),
           M * (3 * C * 4 + 3 * H * DP * 2) + small)
    report("heads_pad_fwd (split only)", lambda: ops.heads_pad_fwd(BF16_F32IN, qkv, 3 * C, qkv[:, C:], 3 * C, qkv[:, 2 * C:],
                                                                   3 * C, None, 0.0, B, T, H, d, out=(qh, kh, vh, None, None, None)),
           M * (3 * C * 4 + 3 * H * DP * 2))
    report("heads_pad_bwd (normalise) ", lambda: ops.heads_pad_bwd(BF16, gh[0], gh[1], gh[2], qh, kh, rq, rk, sqk, 32.0, dqkv,
                                                                   3 * C, dqkv[:, C:], 3 * C, dqkv[:, 2 * C:], 3 * C, B, T, H, d),
           M * C * 2 * 8 + small)
    report("heads_pad_bwd (merge only)", lambda: ops.heads_pad_bwd(BF16, gh[0], gh[1], gh[2], None, None, None, None, None, 0.0,
                                                                   dqkv, 3 * C, dqkv[:, C:], 3 * C, dqkv[:, 2 * C:], 3 * C, B, T,
                                                                   H, d),
           M * C * 2 * 6)
    report("unpad_cols (O)            ", lambda: ops.unpad_cols(o_p, M, H, d, out=o), M * C * 2 * 2)
    report("pad_cols (dO, O)          ", lambda: ops.pad_cols(o, M, H, d, out=o_p), M * (C + H * DP) * 2)


def plain(d):
    C = H * d
    qkv = rn(M, 3 * C)
    sqk = torch.full((C,), 1 / 32, device=dev)
    qh, kh, vh, rq, rk = ops.qknorm_fwd(BF16_F32IN, qkv, 3 * C, qkv[:, C:], 3 * C, qkv[:, 2 * C:], 3 * C, sqk, 32.0, B, T, H, d)
    gh = [rn(B, H, T, d).bfloat16() for _ in range(3)]
    dqkv = torch.empty((M, 3 * C), device=dev, dtype=torch.bfloat16)
    small = 2 * M * H * 4
    print(f"qknorm, d = {d} (C = {C}), M = {M}:")
    report("qknorm_fwd (normalise)    ", lambda: ops.qknorm_fwd(BF16_F32IN, qkv, 3 * C, qkv[:, C:], 3 * C, qkv[:, 2 * C:], 3 * C,
                                                                sqk, 32.0, B, T, H, d), M * C * 18 + small)
    report("qknorm_fwd (split only)   ", lambda: ops.qknorm_fwd(BF16_F32IN, qkv, 3 * C, qkv[:, C:], 3 * C, qkv[:, 2 * C:], 3 * C,
                                                                None, 0.0, B, T, H, d), M * C * 18)
    report("qknorm_bwd (normalise)    ", lambda: ops.qknorm_bwd(BF16, gh[0], gh[1], gh[2], qh, kh, rq, rk, sqk, 32.0, dqkv, 3 * C,
                                                                dqkv[:, C:], 3 * C, dqkv[:, 2 * C:], 3 * C, B, T, H, d),
           M * C * 16 + small)
    report("qknorm_bwd (merge only)   ", lambda: ops.qknorm_bwd(BF16, gh[0], gh[1], gh[2], None, None, None, None, None, 0.0,
                                                                dqkv, 3 * C, dqkv[:, C:], 3 * C, dqkv[:, 2 * C:], 3 * C, B, T,
                                                                H, d), M * C * 12)


padded(80)
for d in (32, 64, 128):
    plain(d)
