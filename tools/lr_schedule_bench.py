#!/usr/bin/env python3
"""What following a learning-rate schedule costs: a constant rate, the host rewriting the rate before every step (the only
way before nvit_amd.LRSchedule), and an LRSchedule attached to the optimizer.

    python tools/lr_schedule_bench.py --out profiles/lr_schedule_bench.log

Legs (bf16): `graphed`, per CONFIG:BATCH of --graphed (default micro_k:512) the replayed `GraphedTrainStep`, variants
(a) constant lr, (b) `set_lr(get_lr(i))` before every replay, (c) schedule attached before the capture; `eager`, per
CONFIG:BATCH of --eager (default base:128) the eager `train_step`, variants (a) constant lr, (b) `group["lr"] = get_lr(i)`
rewritten before every step, (c) schedule attached.  get_lr is the reference's warm-up + cosine; all three variants of a
leg train from the same weights on the same batch.

Arithmetic expectation, printed beside every result: (c) exceeds (a) by one launch of one workgroup (about 3.5 us, what
DropPath's extra launch measured); (b) exceeds (a), replayed, by a drain of the pipeline per step (`set_lr` synchronises
the stream before it touches the staging buffer the graph re-sends, so the host cannot queue the next replay while the
GPU runs this one) and, eager, by an event wait plus a pinned copy.

Every leg is a child process of its own under `timeout` (this process never opens the GPU; a child that hangs ends there),
and the run stops at the first leg that fails.  Inside a leg the variants alternate, a, b, c, a, b, c, ... for --rounds
rounds; a timing is a window of whole calls of at least --window seconds, opened after a warm-up and closed by a device
synchronise, and the figure of a round is window time / calls.  Reported per variant: every round, the median, and the
spread (max - min) / median.  The log (stdout, also written to --out) ends with one LR_SCHEDULE_BENCH JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("graphed", "eager")
LR, MIN_LR, WARMUP, DECAY = 1e-3, 1e-5, 100, 1000000


def window(fn, seconds, sync):
    """ms per call over a window of at least `seconds` (the clock is read every 4 calls; one synchronise at the end, so a
    variant that does not synchronise itself keeps its queue full, as a training loop would)."""
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        if n % 4 == 0 and time.perf_counter() - t0 >= seconds:
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
    from nvit_amd import LRSchedule
    from nvit_amd.config import named_config
    from nvit_amd.model import ViT
    from nvit_amd.train import GraphedTrainStep, train_step
    from nvit_amd.weights import load_formula_weights
    if not torch.cuda.is_available():
        raise SystemExit("lr_schedule_bench: no GPU (a timing needs the MI355X; there is no fallback)")
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    leg = args.worker
    result = {}
    host = LRSchedule.from_reference(LR, MIN_LR, WARMUP, DECAY)   # never moved to the device: lr_at is the host's get_lr

    def images(B, side, C=3):
        g = torch.Generator().manual_seed(B + side)
        return torch.randn(B, C, side, side, generator=g).to(dev)

    def model(cfg, attached):
        m = ViT(cfg)
        load_formula_weights(m, cfg)
        m = m.to(dev).set_precision(args.precision).train()
        opt = m.configure_optimizers(1e-3, LR, (0.9, 0.95), "cuda")
        sched = LRSchedule.from_reference(LR, MIN_LR, WARMUP, DECAY).to(dev) if attached else None
        opt.attach_schedule(sched)
        return m, opt, sched

    for spec in (args.graphed if leg == "graphed" else args.eager):
        name, B = spec.split(":")
        B = int(B)
        cfg = named_config(name)
        X, y = images(B, cfg.image_size, cfg.channels), (torch.arange(B) % cfg.num_classes).to(dev)
        (ma, oa, _), (mb, ob, _), (mc, oc, sched) = model(cfg, False), model(cfg, False), model(cfg, True)
        count = [0]
        if leg == "graphed":
            ga, gb, gc = GraphedTrainStep(ma, oa, X, y), GraphedTrainStep(mb, ob, X, y), GraphedTrainStep(mc, oc, X, y)

            def host_step():
                gb.set_lr(host.lr_at(count[0]))
                count[0] += 1
                gb(X, y)

            variants = {"constant": lambda: ga(X, y), "host_set_lr": host_step, "schedule": lambda: gc(X, y)}
        else:
            def host_step():
                lr = host.lr_at(count[0])
                count[0] += 1
                for group in ob.param_groups:
                    group["lr"] = lr
                train_step(mb, ob, X, y)

            variants = {"constant": lambda: train_step(ma, oa, X, y), "host_set_lr": host_step,
                        "schedule": lambda: train_step(mc, oc, X, y)}
        r = alternate(variants, args, sync)
        base = r["constant"]["median_ms"]
        for k in ("host_set_lr", "schedule"):
            r[k + "_cost_ms"] = round(r[k]["median_ms"] - base, 5)
            r[k + "_cost_rel"] = round(r[k]["median_ms"] / base - 1.0, 5)
        r["expected"] = {"schedule": "one more launch of one workgroup, about 3.5 us",
                         "host_set_lr": ("a stream synchronise per step: the host cannot queue replay i+1 while the GPU runs "
                                         "replay i" if leg == "graphed" else "an event wait and a pinned copy of the lr column")}
        r["schedule_steps"] = sched.step
        r["last_lr"] = [float(sched.last_lr.item()), host.lr_at(sched.step - 1)]
        if abs(r["last_lr"][0] - r["last_lr"][1]) > 1e-7 * LR + 6e-8 * r["last_lr"][1]:
            raise SystemExit(f"lr_schedule_bench: the device schedule left the host's: {r['last_lr']}")
        last = [train_step(m, o, X, y)[1] for m, o in ((ma, oa), (mb, ob), (mc, oc))]
        if not all(torch.isfinite(t).all().item() for t in last):
            raise SystemExit("lr_schedule_bench: non-finite loss")
        result[spec] = r
        print(f"{leg} {spec} {args.precision}: {json.dumps(r)}", flush=True)
        del variants, ma, mb, mc, oa, ob, oc, sched
        if leg == "graphed":
            del ga, gb, gc
        torch.cuda.empty_cache()
    print("LR_SCHEDULE_LEG " + json.dumps({leg: result}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--legs", nargs="*", default=list(LEGS), choices=LEGS)
    ap.add_argument("--eager", nargs="*", default=["base:128"], help="CONFIG:BATCH of the eager-step leg")
    ap.add_argument("--graphed", nargs="*", default=["micro_k:512"], help="CONFIG:BATCH of the replayed-step leg")
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
              "rounds": args.rounds, "precision": args.precision,
              "get_lr": {"lr": LR, "min_lr": MIN_LR, "warmup_iters": WARMUP, "lr_decay_iters": DECAY}}
    log, status = "", 0
    for leg in args.legs:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--worker", leg,
               "--precision", args.precision, "--rounds", str(args.rounds), "--warmup", str(args.warmup),
               "--window", str(args.window), "--graphed", *args.graphed, "--eager", *args.eager]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if not ln.startswith("LR_SCHEDULE_LEG ")]
        part = "\n".join(lines) + "\n"
        done = [ln for ln in r.stdout.splitlines() if ln.startswith("LR_SCHEDULE_LEG ")]
        if r.returncode or not done:   # the first failure ends the run: nothing more is started on the GPU
            part += f"leg {leg}: exit status {r.returncode}\n{r.stderr[-3000:]}\n"
            status = 1
        else:
            result.update(json.loads(done[-1][len("LR_SCHEDULE_LEG "):]))
        print(part, end="", flush=True)
        log += part
        if status:
            break
    if not status:
        tail = "LR_SCHEDULE_BENCH " + json.dumps(result) + "\n"
        print(tail, end="", flush=True)
        log += tail
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(log)
    return status


if __name__ == "__main__":
    sys.exit(main())
