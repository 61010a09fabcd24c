#!/usr/bin/env python3
"""What the on-device RandomResizedCrop + flip and RandomErasing cost: their launches alone, next to the other input
stages, and the train step without and with the full input chain.

    python tools/crop_bench.py --out profiles/crop_bench.log
    python tools/crop_bench.py --crops 512x40x32 --erasings 512x32 --graphed --eager        # a subset

Crop leg, per BxSRCxSIZE (default 512x40x32 and 128x256x224, three channels): `RandomResizedCrop(SIZE)(u8)` = draw + the
two passes of the apply, for each filter, next to `ops.normalize_images` and `AutoAugment` on a uint8 batch of the
output's size, with the bytes a crop has to move (source read once, output written once) and the time they take at the
5.7 TB/s that the row kernels reach: the bar to discuss, not a pass mark.  Erasing leg, per BxSIDE (default 512x32 and
128x224, fp32, three channels): const and pixel in place, pixel out of place, at prob 1.  Step legs (bf16): per CONFIG:BATCH
of --graphed (default micro_k:512) the replayed `GraphedTrainStep` on a tensor against the same on
mix.batch(erase.batch(aug.batch(rrc.batch(u8)))) from a source of 5/4 the side (8/7 at 224: 256); per CONFIG:BATCH of --eager
(default base:128) the eager `train_step` likewise.

One child process under `timeout` does all of it (this process never opens the GPU; a child that hangs ends there).
Inside it the variants of a leg alternate, a, b, a, b, ... for --rounds rounds; a timing is a window of whole calls of
at least --window seconds, opened after a warm-up and closed by a device synchronise, and the figure of a round is
window time / calls.  Reported per variant: every round, the median, and the spread (max - min) / median.  The log
(stdout, also written to --out) ends with one CROP_BENCH JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_KERNEL_TBS = 5.7


def window(fn, seconds, sync):
    """ms per call over a window of at least `seconds` (synchronised every 4 calls and at the end)."""
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        if n % 4 == 0:
            sync()
            if time.perf_counter() - t0 >= seconds:
                break
    sync()
    return (time.perf_counter() - t0) / n * 1e3


def alternate(variants, args, sync):
    """variants: {name: callable}; returns {name: {rounds, median_ms, spread_rel}}."""
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    sync()
    rounds = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            rounds[k].append(round(window(fn, args.window, sync), 5))
    out = {}
    for k, ms in rounds.items():
        med = statistics.median(ms)
        out[k] = {"rounds_ms": ms, "median_ms": med, "spread_rel": round((max(ms) - min(ms)) / med, 4)}
    return out


def source_side(side: int) -> int:
    return 256 if side == 224 else side * 5 // 4


def worker(args) -> None:
    sys.path.insert(0, HERE)
    import torch
    from nvit_amd import ops
    from nvit_amd.augment import AutoAugment
    from nvit_amd.config import named_config
    from nvit_amd.crop import RandomErasing, RandomResizedCrop
    from nvit_amd.mix import Mixup
    from nvit_amd.model import ViT
    from nvit_amd.train import GraphedTrainStep, train_step
    from nvit_amd.weights import load_formula_weights
    if not torch.cuda.is_available():
        raise SystemExit("crop_bench: no GPU (a timing needs the MI355X; there is no fallback)")
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    result = {"what": "ms per call; per variant alternating rounds, median and (max-min)/median", "window_s": args.window,
              "rounds": args.rounds, "precision": args.precision, "crop": {}, "erase": {}, "graphed": {}, "eager": {}}

    def bytes_u8(B, side, C=3, seed=0):
        g = torch.Generator().manual_seed(B + side + seed)
        return torch.randint(0, 256, (B, side, side, C), generator=g, dtype=torch.uint8).to(dev)

    def policy(side):
        return "imagenet" if side >= 128 else "cifar10"

    for spec in args.crops:
        B, src, size = (int(v) for v in spec.split("x"))
        u8, small = bytes_u8(B, src), bytes_u8(B, size, seed=1)
        crops = {f: RandomResizedCrop(size, interpolation=f, seed=1).to(dev) for f in ("bilinear", "bicubic")}
        aug = AutoAugment(policy(size), seed=1).to(dev)
        aug(small)
        r = alternate({"crop+flip bilinear": lambda: crops["bilinear"](u8), "crop+flip bicubic": lambda: crops["bicubic"](u8),
                       "normalize_images": lambda: ops.normalize_images(small), "AutoAugment": lambda: aug(small)}, args, sync)
        moved = u8.numel() + small.numel()
        r["crop_bytes_MB"] = round(moved / 1e6, 3)
        r["crop_bytes_at_row_kernel_rate_ms"] = round(moved / (ROW_KERNEL_TBS * 1e12) * 1e3, 5)
        result["crop"][spec] = r
        print(f"crop {spec}x3: {json.dumps(r)}", flush=True)

    for spec in args.erasings:
        B, side = (int(v) for v in spec.split("x"))
        X = torch.randn(B, 3, side, side, generator=torch.Generator().manual_seed(B + side)).to(dev)
        buf = X.clone()
        const, pixel = (RandomErasing(prob=1.0, mode=m, seed=1).to(dev) for m in ("const", "pixel"))
        r = alternate({"const in place": lambda: const(buf, inplace=True), "pixel in place": lambda: pixel(buf, inplace=True),
                       "pixel out of place": lambda: pixel(X)}, args, sync)
        r["fp32_batch_MB"] = round(X.numel() * 4 / 1e6, 3)
        result["erase"][spec] = r
        print(f"erase {spec}x3: {json.dumps(r)}", flush=True)

    def model(cfg):
        m = ViT(cfg)
        load_formula_weights(m, cfg)
        m = m.to(dev).set_precision(args.precision).train()
        return m, m.configure_optimizers(1e-3, 1e-3, (0.9, 0.95), "cuda")

    for leg, specs in (("graphed", args.graphed), ("eager", args.eager)):
        for spec in specs:
            name, B = spec.split(":")
            B = int(B)
            cfg = named_config(name)
            side = cfg.image_size
            X = torch.randn(B, cfg.channels, side, side, generator=torch.Generator().manual_seed(B)).to(dev)
            u8, y = bytes_u8(B, source_side(side), cfg.channels), (torch.arange(B) % cfg.num_classes).to(dev)
            rrc = RandomResizedCrop(side, interpolation="bicubic", seed=1).to(dev)
            aug, erase, mix = AutoAugment(policy(side), seed=2).to(dev), RandomErasing(seed=3).to(dev), Mixup(seed=4).to(dev)

            def chain():
                return mix.batch(erase.batch(aug.batch(rrc.batch(u8))))

            (mp, op_), (mc, oc) = model(cfg), model(cfg)
            if leg == "graphed":
                plain, chained = GraphedTrainStep(mp, op_, X, y), GraphedTrainStep(mc, oc, chain(), y)
                variants = {"step": lambda: plain(X, y), "step+chain": lambda: chained(u8, y)}
            else:
                variants = {"step": lambda: train_step(mp, op_, X, y), "step+chain": lambda: train_step(mc, oc, chain(), y)}
            r = alternate(variants, args, sync)
            r["chain_cost_rel"] = round(r["step+chain"]["median_ms"] / r["step"]["median_ms"] - 1.0, 5)
            r["source"] = f"{source_side(side)}x{source_side(side)}x{cfg.channels} uint8"
            last = [train_step(mp, op_, X, y)[1], train_step(mc, oc, chain(), y)[1]]
            if not all(torch.isfinite(t).all().item() for t in last):
                raise SystemExit("crop_bench: non-finite loss")
            result[leg][spec] = r
            print(f"{leg} {spec} {args.precision}: {json.dumps(r)}", flush=True)
            del variants, mp, mc, op_, oc
            if leg == "graphed":
                del plain, chained
            torch.cuda.empty_cache()
    print("CROP_BENCH " + json.dumps(result), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--crops", nargs="*", default=["512x40x32", "128x256x224"], help="BxSRCxSIZE of the crop leg")
    ap.add_argument("--erasings", nargs="*", default=["512x32", "128x224"], help="BxSIDE of the erasing leg")
    ap.add_argument("--graphed", nargs="*", default=["micro_k:512"], help="CONFIG:BATCH of the replayed-step leg")
    ap.add_argument("--eager", nargs="*", default=["base:128"], help="CONFIG:BATCH of the eager-step leg")
    ap.add_argument("--precision", default="bf16", choices=("bf16", "fp32"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls of every variant ahead of the rounds")
    ap.add_argument("--window", type=float, default=1.0, help="least seconds of a timed window")
    ap.add_argument("--timeout", type=int, default=420, help="time limit of the child process, seconds")
    ap.add_argument("--out", default=None, help="also write the log to this file")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        worker(args)
        return 0
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--worker",
           "--precision", args.precision, "--rounds", str(args.rounds), "--warmup", str(args.warmup),
           "--window", str(args.window), "--crops", *args.crops, "--erasings", *args.erasings, "--graphed", *args.graphed,
           "--eager", *args.eager]
    r = subprocess.run(cmd, capture_output=True, text=True)
    log = r.stdout + (f"\nexit status {r.returncode}\n{r.stderr[-3000:]}" if r.returncode else "")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(log)
    print(log, end="")
    return 0 if r.returncode == 0 and "CROP_BENCH " in r.stdout else 1


if __name__ == "__main__":
    sys.exit(main())
