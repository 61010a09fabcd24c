"""Attention throughput per head dim at a Base-sized shape: B = 128, T = 784, H * d = 768 (H = 24, 12, 6 for d = 32, 64,
128).  For each d: the forward (bounded-score entry point and generic entry point) and the unfused backward, on the MFMA
kernels (impl 1) and on the scalar-FMA kernels (impl 0), bf16 operands.  The two implementations run in interleaved
rounds; each timing is device events around `iters` back-to-back calls after a warm-up; the table reports the median
over rounds in ms per call and TFLOP/s from the algorithmic counts of ProfScope (4 B H T^2 d forward, 10 B H T^2 d
backward).  The bounded forward uses the training path's q pre-scale (attn_q_prescale(d)), scores inside the fast-path
range.

    python tools/attn_headdim_bench.py [--rounds 5] [--iters 20] [--json out.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nvit_amd import ops  # noqa: E402
from nvit_amd._lib import BF16  # noqa: E402

B, T, C = 128, 784, 768
DIMS = (32, 64, 128)
OPS = ("fwd_bounded", "fwd", "bwd")


def flops(op, d):
    H = C // d
    return (10.0 if op == "bwd" else 4.0) * B * H * T * T * d


def make(d, dev):
    H = C // d
    g = torch.Generator().manual_seed(d)
    sqk = (1.0 / 32.0) * (1.0 + 0.3 * torch.tanh(torch.randn(C, generator=g)))
    s_eff = (sqk * 32.0).reshape(1, H, 1, d)
    nrm = torch.nn.functional.normalize
    qpre = ops.attn_q_prescale(d)
    q = (s_eff * nrm(torch.randn(B, H, T, d, generator=g), dim=-1)).bfloat16().to(dev)
    qp = (qpre * s_eff * nrm(torch.randn(B, H, T, d, generator=g), dim=-1)).bfloat16().to(dev)
    k = (s_eff * nrm(torch.randn(B, H, T, d, generator=g), dim=-1)).bfloat16().to(dev)
    v = torch.randn(B, H, T, d, generator=g).bfloat16().to(dev)
    do = torch.randn(B * T, C, generator=g).bfloat16().to(dev)
    return dict(q=q, qp=qp, k=k, v=v, do=do, sqk=sqk.to(dev), qpre=qpre, scale=math.sqrt(d))


def call(op, impl, x):
    if op == "fwd_bounded":
        return ops.attn_fwd(BF16, impl, x["qp"], x["k"], x["v"], x["scale"], x["sqk"], 32.0, q_prescale=x["qpre"])
    if op == "fwd":
        return ops.attn_fwd(BF16, impl, x["q"], x["k"], x["v"], x["scale"])
    return ops.attn_bwd(BF16, impl, x["do"], x["q"], x["k"], x["v"], x["o"][impl], x["lse"][impl], x["scale"])


def timed(op, impl, x, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call(op, impl, x)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20, help="calls per timing on the MFMA kernels (a quarter on impl 0)")
    ap.add_argument("--json", default=None)
    ap.add_argument("--impls", default="1,0", help="implementations to time (1 alone: for a profiler run)")
    a = ap.parse_args()
    impls = tuple(int(i) for i in a.impls.split(","))
    dev = torch.device("cuda:0")
    print(f"# {torch.cuda.get_device_name(0)}  B={B} T={T} H*d={C}  rounds={a.rounds} iters={a.iters}")
    data = {d: make(d, dev) for d in DIMS}
    for d, x in data.items():   # attention outputs for the backward, per implementation; doubles as the warm-up
        x["o"], x["lse"] = {}, {}
        for impl in impls:
            x["o"][impl], x["lse"][impl] = ops.attn_fwd(BF16, impl, x["q"], x["k"], x["v"], x["scale"])
            for op in OPS:
                call(op, impl, x)
    torch.cuda.synchronize()
    ms = {(d, impl, op): [] for d in DIMS for impl in impls for op in OPS}
    for _ in range(a.rounds):
        for d in DIMS:
            for op in OPS:
                for impl in impls:
                    ms[(d, impl, op)].append(timed(op, impl, data[d], a.iters if impl == 1 else max(1, a.iters // 4)))
    rows = []
    print(f"{'d':>4} {'H':>3} {'op':>12} {'impl':>5} {'ms':>9} {'spread%':>8} {'TFLOP/s':>8} {'mfma/scalar':>12}")
    for d in DIMS:
        for op in OPS:
            med = {impl: statistics.median(ms[(d, impl, op)]) for impl in impls}
            for impl in impls:
                v = ms[(d, impl, op)]
                spread = 100.0 * (max(v) - min(v)) / med[impl]
                tf = flops(op, d) / (med[impl] * 1e-3) / 1e12
                ratio = med[0] / med[1] if 0 in med and 1 in med else float("nan")
                rows.append(dict(d=d, H=C // d, op=op, impl=impl, ms=med[impl], spread_pct=spread, tflops=tf,
                                 speedup_vs_scalar=ratio if impl == 1 else None))
                print(f"{d:>4} {C // d:>3} {op:>12} {impl:>5} {med[impl]:>9.3f} {spread:>8.1f} {tf:>8.1f} "
                      f"{(f'{ratio:.1f}x' if impl == 1 else ''):>12}")
    if 1 not in impls:
        return
    m64 = {op: next(r["tflops"] for r in rows if r["d"] == 64 and r["impl"] == 1 and r["op"] == op) for op in OPS}
    for d in (32, 128):
        rel = ", ".join(f"{op} {next(r['tflops'] for r in rows if r['d'] == d and r['impl'] == 1 and r['op'] == op) / m64[op]:.2f}"
                        for op in OPS)
        print(f"# MFMA TFLOP/s at d = {d} relative to d = 64: {rel}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(B=B, T=T, C=C, rounds=a.rounds, iters=a.iters, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
