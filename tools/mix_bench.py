#!/usr/bin/env python3
"""What the on-device Mixup / CutMix costs: the two launches alone, and the train step with and without them.

    python tools/mix_bench.py --out profiles/mix_bench.log
    python tools/mix_bench.py --pipelines 512x32 --graphed micro_k:512 --eager        # a subset

Pipeline leg, per BxSIDE (default 512x32 and 128x224, three channels, fp32): `Mixup()(X, y)` = nvit_mix_draw +
nvit_mix_apply, out of place and in place.  Step legs (bf16): per CONFIG:BATCH of --graphed (default micro_k:512) the
replayed `GraphedTrainStep` on X against the same on `mix.batch(X)`; per CONFIG:BATCH of --eager (default base:128) the
eager `train_step` likewise.  A last leg records the error of nvit_ce_loss_soft and of nvit_ce_loss against fp64 torch
at the shapes of tests/test_gpu_mix.py.

One child process under `timeout` does all of it (this process never opens the GPU; a child that hangs ends there).
Inside it the variants of a leg alternate, a, b, a, b, ... for --rounds rounds; a timing is a window of whole calls of
at least --window seconds, opened after a warm-up and closed by a device synchronise, and the figure of a round is
window time / calls.  Reported per variant: every round, the median, and the spread (max - min) / median.  The log
(stdout, also written to --out) ends with one MIX_BENCH JSON line.
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


def loss_errors(torch, dev):
    """Errors of the soft and the hard loss kernel against fp64 torch (loss absolute, dlogits max absolute)."""
    from nvit_amd.mix import MixedTargets
    from nvit_amd.train import CrossEntropyFn
    F = torch.nn.functional
    out = {}
    for B, N in ((3, 7), (8, 10), (33, 100), (128, 1000)):
        g = torch.Generator().manual_seed(6)
        logits = torch.randn(B, N, generator=torch.Generator().manual_seed(5)) * 3.0
        y, y2 = torch.randint(0, N, (B,), generator=g), torch.randint(0, N, (B,), generator=g)
        lam = torch.rand(B, generator=g)
        lam[0], lam[1] = 0.0, 1.0
        row = {}
        for eps in (None, 0.0, 0.1):   # None: the hard loss
            l64 = logits.double().requires_grad_(True)
            if eps is None:
                ref = F.cross_entropy(l64, y)
                target = y.to(dev)
            else:
                t = torch.zeros(B, N, dtype=torch.float64)
                t[torch.arange(B), y] += lam.double()
                t[torch.arange(B), y2] += 1.0 - lam.double()
                ref = F.cross_entropy(l64, (1.0 - eps) * t + eps / N)
                target = MixedTargets(y.to(dev), y2.to(dev), lam.to(dev), eps)
            ref.backward()
            lg = logits.to(dev).requires_grad_(True)
            got = CrossEntropyFn.apply(lg, target)
            got.backward()
            row["hard" if eps is None else f"soft eps={eps}"] = {
                "loss_err": abs(got.item() - ref.item()), "dlogits_err": (lg.grad.cpu().double() - l64.grad).abs().max().item()}
        out[f"{B}x{N}"] = row
    return out


def worker(args) -> None:
    sys.path.insert(0, HERE)
    import torch
    from nvit_amd.config import named_config
    from nvit_amd.mix import Mixup
    from nvit_amd.model import ViT
    from nvit_amd.train import GraphedTrainStep, train_step
    from nvit_amd.weights import load_formula_weights
    if not torch.cuda.is_available():
        raise SystemExit("mix_bench: no GPU (a timing needs the MI355X; there is no fallback)")
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    result = {"what": "ms per call; per variant alternating rounds, median and (max-min)/median", "window_s": args.window,
              "rounds": args.rounds, "precision": args.precision, "pipeline": {}, "graphed": {}, "eager": {}}

    def images(B, side, C=3):
        g = torch.Generator().manual_seed(B + side)
        return torch.randn(B, C, side, side, generator=g).to(dev)

    for spec in args.pipelines:
        B, side = (int(v) for v in spec.split("x"))
        X, y = images(B, side), (torch.arange(B) % 10).to(dev)
        buf = X.clone()
        mix = Mixup(seed=1).to(dev)
        r = alternate({"draw+apply": lambda: mix(X, y), "draw+apply in place": lambda: mix(buf, y, inplace=True)}, args, sync)
        r["fp32_batch_MB"] = round(X.numel() * 4 / 1e6, 3)
        result["pipeline"][spec] = r
        print(f"pipeline {spec}x3: {json.dumps(r)}", flush=True)

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
            X, y = images(B, cfg.image_size, cfg.channels), (torch.arange(B) % cfg.num_classes).to(dev)
            mix = Mixup(seed=1).to(dev)
            (mp, op_), (mm, om) = model(cfg), model(cfg)
            if leg == "graphed":
                plain, mixed = GraphedTrainStep(mp, op_, X, y), GraphedTrainStep(mm, om, mix.batch(X), y)
                variants = {"step": lambda: plain(X, y), "step+mix": lambda: mixed(X, y)}
            else:
                variants = {"step": lambda: train_step(mp, op_, X, y), "step+mix": lambda: train_step(mm, om, mix.batch(X), y)}
            r = alternate(variants, args, sync)
            r["mix_cost_rel"] = round(r["step+mix"]["median_ms"] / r["step"]["median_ms"] - 1.0, 5)
            last = [train_step(mp, op_, X, y)[1], train_step(mm, om, mix.batch(X), y)[1]]
            if not all(torch.isfinite(t).all().item() for t in last):
                raise SystemExit("mix_bench: non-finite loss")
            result[leg][spec] = r
            print(f"{leg} {spec} {args.precision}: {json.dumps(r)}", flush=True)
            del variants, mp, mm, op_, om
            if leg == "graphed":
                del plain, mixed
            torch.cuda.empty_cache()
    result["loss_error_vs_fp64"] = loss_errors(torch, dev)
    print(f"loss errors against fp64: {json.dumps(result['loss_error_vs_fp64'])}", flush=True)
    print("MIX_BENCH " + json.dumps(result), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pipelines", nargs="*", default=["512x32", "128x224"], help="BxSIDE of the pipeline leg")
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
           "--window", str(args.window), "--pipelines", *args.pipelines, "--graphed", *args.graphed, "--eager", *args.eager]
    r = subprocess.run(cmd, capture_output=True, text=True)
    log = r.stdout + (f"\nexit status {r.returncode}\n{r.stderr[-3000:]}" if r.returncode else "")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(log)
    print(log, end="")
    return 0 if r.returncode == 0 and "MIX_BENCH " in r.stdout else 1


if __name__ == "__main__":
    sys.exit(main())
