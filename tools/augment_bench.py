#!/usr/bin/env python3
"""What the on-device AutoAugment costs: the input pipeline alone, and the train step with and without it.

    python tools/augment_bench.py --out profiles/augment_bench.log
    python tools/augment_bench.py --pipelines 512x32 --steps micro_k:512        # a subset

Pipeline leg, per BxSIDE (default 512x32 and 128x224, three channels): (a) `ops.normalize_images(u8)`, the whole input
pipeline without augmentation, against (b) `AutoAugment(policy)(u8)` = nvit_augment_draw + nvit_augment_apply.
Step leg, per CONFIG:BATCH (default micro_k:512 and base:128, bf16): `train_step` and `GraphedTrainStep` on the fp32
batch against the same on `aug.batch(u8)`.

One child process under `timeout` does all of it (this process never opens the GPU; a child that hangs ends there).
Inside it the variants of a leg alternate, a, b, a, b, ... for --rounds rounds; a timing is a window of whole calls of
at least --window seconds, opened after a warm-up and closed by a device synchronise, and the figure of a round is
window time / calls.  Reported per variant: every round, the median, and the spread (max - min) / median.  The log
(stdout, also written to --out) ends with one AUGMENT_BENCH JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def worker(args) -> None:
    sys.path.insert(0, HERE)
    import torch
    from nvit_amd import ops
    from nvit_amd.augment import AutoAugment
    from nvit_amd.config import named_config
    from nvit_amd.model import ViT
    from nvit_amd.train import GraphedTrainStep, train_step
    from nvit_amd.weights import load_formula_weights
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench: no GPU (a timing needs the MI355X; there is no fallback)")
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    result = {"what": "ms per call; per variant three alternating rounds, median and (max-min)/median",
              "policy": args.policy, "window_s": args.window, "rounds": args.rounds, "pipeline": {}, "step": {}}

    def batch_u8(B, side, C=3):
        g = torch.Generator().manual_seed(B + side)
        return torch.randint(0, 256, (B, side, side, C), generator=g, dtype=torch.uint8).to(dev)

    for spec in args.pipelines:
        B, side = (int(v) for v in spec.split("x"))
        u8 = batch_u8(B, side)
        aug = AutoAugment(args.policy, seed=1).to(dev)
        r = alternate({"normalize_images": lambda: ops.normalize_images(u8), "draw+apply": lambda: aug(u8)}, args, sync)
        r["augment_minus_normalize_ms"] = round(r["draw+apply"]["median_ms"] - r["normalize_images"]["median_ms"], 5)
        result["pipeline"][spec] = r
        print(f"pipeline {spec}x3: {json.dumps(r)}", flush=True)

    for spec in args.steps:
        name, B = spec.split(":")
        B = int(B)
        cfg = named_config(name)
        u8 = batch_u8(B, cfg.image_size, cfg.channels)
        X = ops.normalize_images(u8)
        y = (torch.arange(B) % cfg.num_classes).to(dev)

        def model():
            m = ViT(cfg)
            load_formula_weights(m, cfg)
            m = m.to(dev).set_precision(args.precision).train()
            return m, m.configure_optimizers(1e-3, 1e-3, (0.9, 0.95), "cuda")

        aug_e, aug_g = (AutoAugment(args.policy, seed=1).to(dev) for _ in range(2))
        (me, oe), (mg, og), (ma, oa) = model(), model(), model()
        plain = GraphedTrainStep(mg, og, X, y)
        graphed = GraphedTrainStep(ma, oa, aug_g.batch(u8), y)
        r = alternate({"eager": lambda: train_step(me, oe, X, y),
                       "eager+augment": lambda: train_step(me, oe, aug_e.batch(u8), y),
                       "graphed": lambda: plain(X, y),
                       "graphed+augment": lambda: graphed(u8, y)}, args, sync)
        for k in ("eager", "graphed"):
            r[k + "_augment_cost_rel"] = round(r[k + "+augment"]["median_ms"] / r[k]["median_ms"] - 1.0, 5)
        if not all(torch.isfinite(t).all().item() for t in (plain.loss, graphed.loss)):
            raise SystemExit("augment_bench: non-finite loss")
        result["step"][spec] = r
        print(f"step {spec} {args.precision}: {json.dumps(r)}", flush=True)
        del plain, graphed, me, mg, ma, oe, og, oa
        torch.cuda.empty_cache()
    print("AUGMENT_BENCH " + json.dumps(result), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pipelines", nargs="*", default=["512x32", "128x224"], help="BxSIDE of the pipeline leg")
    ap.add_argument("--steps", nargs="*", default=["micro_k:512", "base:128"], help="CONFIG:BATCH of the step leg")
    ap.add_argument("--policy", default="cifar10")
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
           "--policy", args.policy, "--precision", args.precision, "--rounds", str(args.rounds), "--warmup", str(args.warmup),
           "--window", str(args.window), "--pipelines", *args.pipelines, "--steps", *args.steps]
    r = subprocess.run(cmd, capture_output=True, text=True)
    log = r.stdout + (f"\nexit status {r.returncode}\n{r.stderr[-3000:]}" if r.returncode else "")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(log)
    print(log, end="")
    return 0 if r.returncode == 0 and "AUGMENT_BENCH " in r.stdout else 1


if __name__ == "__main__":
    sys.exit(main())
