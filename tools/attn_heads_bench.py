"""Forward / backward time of the head-axis attention kernels (flash_attn=True; nvit_attn_heads_fwd / _bwd) at the
shapes of a Base and a Large step, with the effective bandwidth of their algorithmic traffic (each input read once,
each output written once).

Usage:  python tools/attn_heads_bench.py [--iters N]
Prints one line per (shape, mode) and a JSON summary line."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from nvit_amd import ops
from nvit_amd._lib import BF16, F32

SHAPES = [("base_B128", 128 * 784, 12, 64), ("large_B64", 64 * 784, 16, 64)]


def _time(fn, iters):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters   # microseconds


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    out = []
    for name, M, H, d in SHAPES:
        C = H * d
        qkv = torch.randn(M, 3 * C, device="cuda")
        sqk = torch.full((C,), 1.0 / math.sqrt(C), device="cuda")
        c_q = math.sqrt(C)
        for dt in (BF16, F32):
            es = 2 if dt == BF16 else 4
            td = ops.tdtype(dt)
            q, k, v = qkv, qkv[:, C:], qkv[:, 2 * C:]
            o, lse = ops.attn_heads_fwd(dt, q, 3 * C, k, v, 3 * C, sqk, c_q, math.sqrt(d), M, H, d)
            dout = torch.randn(M, C, device="cuda").to(td)
            dqkv = torch.empty(M, 3 * C, device="cuda", dtype=td)
            fwd = lambda: ops.attn_heads_fwd(dt, q, 3 * C, k, v, 3 * C, sqk, c_q, math.sqrt(d), M, H, d)
            bwd = lambda: ops.attn_heads_bwd(dt, dout, q, 3 * C, k, v, 3 * C, sqk, c_q, math.sqrt(d), lse, dqkv, 3 * C,
                                             dqkv[:, C:], dqkv[:, 2 * C:], 3 * C, M, H, d)
            tf, tb = _time(fwd, args.iters), _time(bwd, args.iters)
            bf = M * (3 * C * 4 + C * es + H * 4)                       # q, k, v fp32 in; O, lse out
            bb = M * (3 * C * 4 + C * es + H * 4 + 3 * C * es)          # q, k, v, dO, lse in; dq, dk, dv out
            rec = dict(shape=name, mode="bf16" if dt == BF16 else "fp32", M=M, H=H, d=d, fwd_us=round(tf, 1),
                       fwd_TBps=round(bf / tf / 1e6, 2), bwd_us=round(tb, 1), bwd_TBps=round(bb / tb / 1e6, 2))
            print(f"{name:10s} {rec['mode']}: fwd {tf:8.1f} us {rec['fwd_TBps']:5.2f} TB/s   "
                  f"bwd {tb:8.1f} us {rec['bwd_TBps']:5.2f} TB/s", flush=True)
            out.append(rec)
    print(json.dumps({"attn_heads": out}))


if __name__ == "__main__":
    main()
