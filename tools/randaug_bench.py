#!/usr/bin/env python3
"""What the on-device RandAugment costs next to AutoAugment: the input pipeline alone, and the train step with either.

    python tools/randaug_bench.py --out profiles/randaug_bench.log
    python tools/randaug_bench.py --pipelines 512x32 --steps micro_k:512        # a subset

Pipeline leg, per BxSIDE (default 512x32 and 128x224, three channels): `ops.normalize_images(u8)`, the whole input
pipeline without augmentation, against `AutoAugment(policy)(u8)` and `RandAugment.from_config(config)(u8)` (draw + apply
each).  Step leg, per CONFIG:BATCH:MODE (default micro_k:512:graphed and base:128:eager, bf16): the step on the fp32
batch, on `aug.batch(u8)` and on `ra.batch(u8)`.

One child process under `timeout` does all of it (this process never opens the GPU; a child that hangs ends there).
Inside it the variants of a leg alternate, a, b, c, a, b, c, ... for --rounds rounds; a timing is a window of whole calls
of at least --window seconds, opened after a warm-up and closed by a device synchronise, and the figure of a round is
window time / calls.  Reported per variant: every round, the median, and the spread (max - min) / median.  The log
(stdout, also written to --out) ends with one RANDAUG_BENCH JSON line.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
from augment_bench import alternate  # noqa: E402  (the windowed, alternating timing of the AutoAugment bench)


def worker(args) -> None:
    sys.path.insert(0, HERE)
    import torch
    from nvit_amd import ops
    from nvit_amd.augment import AutoAugment
    from nvit_amd.config import named_config
    from nvit_amd.model import ViT
    from nvit_amd.randaug import RandAugment
    from nvit_amd.train import GraphedTrainStep, train_step
    from nvit_amd.weights import load_formula_weights
    if not torch.cuda.is_available():
        raise SystemExit("randaug_bench: no GPU (a timing needs the MI355X; there is no fallback)")
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    result = {"what": "ms per call; per variant alternating rounds, median and (max-min)/median", "policy": args.policy,
              "config": args.config, "interpolation": args.interpolation, "window_s": args.window, "rounds": args.rounds,
              "pipeline": {}, "step": {}}

    def batch_u8(B, side, C=3):
        g = torch.Generator().manual_seed(B + side)
        return torch.randint(0, 256, (B, side, side, C), generator=g, dtype=torch.uint8).to(dev)

    def rand_augment():
        return RandAugment.from_config(args.config, interpolation=args.interpolation, fill=(124, 116, 104), seed=1).to(dev)

    for spec in args.pipelines:
        B, side = (int(v) for v in spec.split("x"))
        u8 = batch_u8(B, side)
        aug, ra = AutoAugment(args.policy, seed=1).to(dev), rand_augment()
        r = alternate({"normalize_images": lambda: ops.normalize_images(u8), "AutoAugment": lambda: aug(u8),
                       "RandAugment": lambda: ra(u8)}, args, sync)
        for k in ("AutoAugment", "RandAugment"):
            r[k + "_minus_normalize_ms"] = round(r[k]["median_ms"] - r["normalize_images"]["median_ms"], 5)
        result["pipeline"][spec] = r
        print(f"pipeline {spec}x3: {json.dumps(r)}", flush=True)

    for spec in args.steps:
        name, B, mode = spec.split(":")
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

        aug, ra = AutoAugment(args.policy, seed=1).to(dev), rand_augment()
        if mode == "graphed":
            (mp, op_), (ma, oa), (mr, or_) = model(), model(), model()
            plain = GraphedTrainStep(mp, op_, X, y)
            with_aa = GraphedTrainStep(ma, oa, aug.batch(u8), y)
            with_ra = GraphedTrainStep(mr, or_, ra.batch(u8), y)
            variants = {"plain": lambda: plain(X, y), "AutoAugment": lambda: with_aa(u8, y), "RandAugment": lambda: with_ra(u8, y)}
            losses = lambda: (plain.loss, with_aa.loss, with_ra.loss)  # noqa: E731
        elif mode == "eager":
            m, o = model()
            last = {}

            def step(key, x):
                last[key] = train_step(m, o, x, y)[1]
            variants = {"plain": lambda: step("plain", X), "AutoAugment": lambda: step("aa", aug.batch(u8)),
                        "RandAugment": lambda: step("ra", ra.batch(u8))}
            losses = lambda: tuple(last.values())  # noqa: E731
        else:
            raise SystemExit(f"randaug_bench: mode is graphed or eager (got {mode!r})")
        r = alternate(variants, args, sync)
        for k in ("AutoAugment", "RandAugment"):
            r[k + "_cost_rel"] = round(r[k]["median_ms"] / r["plain"]["median_ms"] - 1.0, 5)
        if not all(torch.isfinite(t).all().item() for t in losses()):
            raise SystemExit("randaug_bench: non-finite loss")
        result["step"][spec] = r
        print(f"step {spec} {args.precision}: {json.dumps(r)}", flush=True)
        del variants
        torch.cuda.empty_cache()
    print("RANDAUG_BENCH " + json.dumps(result), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pipelines", nargs="*", default=["512x32", "128x224"], help="BxSIDE of the pipeline leg")
    ap.add_argument("--steps", nargs="*", default=["micro_k:512:graphed", "base:128:eager"], help="CONFIG:BATCH:MODE of the step leg")
    ap.add_argument("--policy", default="cifar10", help="AutoAugment's policy")
    ap.add_argument("--config", default="rand-m9-mstd0.5-inc1", help="RandAugment's timm string")
    ap.add_argument("--interpolation", default="random", choices=("random", "bilinear", "bicubic"))
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
           "--policy", args.policy, "--config", args.config, "--interpolation", args.interpolation, "--precision", args.precision,
           "--rounds", str(args.rounds), "--warmup", str(args.warmup), "--window", str(args.window),
           "--pipelines", *args.pipelines, "--steps", *args.steps]
    r = subprocess.run(cmd, capture_output=True, text=True)
    log = r.stdout + (f"\nexit status {r.returncode}\n{r.stderr[-3000:]}" if r.returncode else "")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(log)
    print(log, end="")
    return 0 if r.returncode == 0 and "RANDAUG_BENCH " in r.stdout else 1


if __name__ == "__main__":
    sys.exit(main())
