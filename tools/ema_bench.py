#!/usr/bin/env python3
"""What the on-device weight EMA (nvit_amd.ModelEma) costs: the train step without and with an attached EMA, and its two
calls alone.

    python tools/ema_bench.py --out profiles/ema_bench.log
    python tools/ema_bench.py --legs graphed alone            # a subset

Legs (bf16): `graphed`, per CONFIG:BATCH of --graphed (default micro_k:512) the replayed `GraphedTrainStep` of a model
without and of a model with an EMA attached before the capture; `eager`, per CONFIG:BATCH of --eager (default base:128)
the eager `train_step` likewise; `alone`, per CONFIG of --alone (default base) `ema.update()` (tick + table launch) and
`ema.sync()` (copy launch + normalize_matrices of the module) on their own, with the bytes they move (12 B and 8 B per
averaged parameter) and the rate that gives.

Every leg is a child process of its own under `timeout` (this process never opens the GPU; a child that hangs ends
there), and the run stops at the first leg that fails.  Inside a leg the variants alternate, a, b, a, b, ... for
--rounds rounds; a timing is a window of whole calls of at least --window seconds, opened after a warm-up and closed by a
device synchronise, and the figure of a round is window time / calls.  Reported per variant: every round, the median,
and the spread (max - min) / median.  The log (stdout, also written to --out) ends with one EMA_BENCH JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("graphed", "eager", "alone")


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
    from nvit_amd.config import named_config
    from nvit_amd.ema import ModelEma
    from nvit_amd.model import ViT
    from nvit_amd.train import GraphedTrainStep, train_step
    from nvit_amd.weights import load_formula_weights
    if not torch.cuda.is_available():
        raise SystemExit("ema_bench: no GPU (a timing needs the MI355X; there is no fallback)")
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    leg = args.worker
    result = {}

    def images(B, side, C=3):
        g = torch.Generator().manual_seed(B + side)
        return torch.randn(B, C, side, side, generator=g).to(dev)

    def model(cfg, with_ema):
        m = ViT(cfg)
        load_formula_weights(m, cfg)
        m = m.to(dev).set_precision(args.precision).train()
        opt = m.configure_optimizers(1e-3, 1e-3, (0.9, 0.95), "cuda")
        ema = ModelEma(m) if with_ema else None
        opt.attach_ema(ema)
        return m, opt, ema

    if leg in ("graphed", "eager"):
        for spec in (args.graphed if leg == "graphed" else args.eager):
            name, B = spec.split(":")
            B = int(B)
            cfg = named_config(name)
            X, y = images(B, cfg.image_size, cfg.channels), (torch.arange(B) % cfg.num_classes).to(dev)
            (mp, op_, _), (me, oe, ema) = model(cfg, False), model(cfg, True)
            if leg == "graphed":
                plain, averaged = GraphedTrainStep(mp, op_, X, y), GraphedTrainStep(me, oe, X, y)
                variants = {"step": lambda: plain(X, y), "step+ema": lambda: averaged(X, y)}
            else:
                variants = {"step": lambda: train_step(mp, op_, X, y), "step+ema": lambda: train_step(me, oe, X, y)}
            r = alternate(variants, args, sync)
            r["ema_cost_rel"] = round(r["step+ema"]["median_ms"] / r["step"]["median_ms"] - 1.0, 5)
            r["ema_cost_ms"] = round(r["step+ema"]["median_ms"] - r["step"]["median_ms"], 5)
            r["averaged_parameters"] = sum(t.numel() for t in ema.shadow.values())
            r["updates"] = ema.updates
            last = [train_step(mp, op_, X, y)[1], train_step(me, oe, X, y)[1]]
            if not all(torch.isfinite(t).all().item() for t in last):
                raise SystemExit("ema_bench: non-finite loss")
            if not all(torch.isfinite(t).all().item() for t in ema.shadow.values()):
                raise SystemExit("ema_bench: non-finite average")
            result[spec] = r
            print(f"{leg} {spec} {args.precision}: {json.dumps(r)}", flush=True)
            del variants, mp, me, op_, oe, ema
            if leg == "graphed":
                del plain, averaged
            torch.cuda.empty_cache()
    else:
        for name in args.alone:
            cfg = named_config(name)
            m, opt, ema = model(cfg, True)
            n = sum(t.numel() for t in ema.shadow.values())
            r = alternate({"update": ema.update, "sync": ema.sync}, args, sync)
            r["averaged_parameters"], r["renorm"] = n, ema.renorm
            r["update_GB"], r["sync_copy_GB"] = round(12 * n / 1e9, 4), round(8 * n / 1e9, 4) if ema.renorm else 0.0
            r["update_TB_per_s"] = round(12 * n / 1e12 / (r["update"]["median_ms"] / 1e3), 3)
            result[name] = r
            print(f"alone {name}: {json.dumps(r)}", flush=True)
            del m, opt, ema
            torch.cuda.empty_cache()
    print("EMA_LEG " + json.dumps({leg: result}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--legs", nargs="*", default=list(LEGS), choices=LEGS)
    ap.add_argument("--graphed", nargs="*", default=["micro_k:512"], help="CONFIG:BATCH of the replayed-step leg")
    ap.add_argument("--eager", nargs="*", default=["base:128"], help="CONFIG:BATCH of the eager-step leg")
    ap.add_argument("--alone", nargs="*", default=["base"], help="CONFIG of the update() / sync() leg")
    ap.add_argument("--precision", default="bf16", choices=("bf16", "fp32"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls of every variant ahead of the rounds")
    ap.add_argument("--window", type=float, default=1.0, help="least seconds of a timed window")
    ap.add_argument("--timeout", type=int, default=240, help="time limit of each leg's child process, seconds")
    ap.add_argument("--out", default=None, help="also write the log to this file")
    ap.add_argument("--worker", default=None, choices=LEGS, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        worker(args)
        return 0
    result = {"what": "ms per call; per variant alternating rounds, median and (max-min)/median", "window_s": args.window,
              "rounds": args.rounds, "precision": args.precision}
    log, status = "", 0
    for leg in args.legs:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--worker", leg,
               "--precision", args.precision, "--rounds", str(args.rounds), "--warmup", str(args.warmup),
               "--window", str(args.window), "--graphed", *args.graphed, "--eager", *args.eager, "--alone", *args.alone]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if not ln.startswith("EMA_LEG ")]
        part = "\n".join(lines) + "\n"
        done = [ln for ln in r.stdout.splitlines() if ln.startswith("EMA_LEG ")]
        if r.returncode or not done:   # the first failure ends the run: nothing more is started on the GPU
            part += f"leg {leg}: exit status {r.returncode}\n{r.stderr[-3000:]}\n"
            status = 1
        else:
            result.update(json.loads(done[-1][len("EMA_LEG "):]))
        print(part, end="", flush=True)
        log += part
        if status:
            break
    if not status:
        tail = "EMA_BENCH " + json.dumps(result) + "\n"
        print(tail, end="", flush=True)
        log += tail
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(log)
    return status


if __name__ == "__main__":
    sys.exit(main())
