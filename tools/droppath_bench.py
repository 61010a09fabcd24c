#!/usr/bin/env python3
"""What stochastic depth (nvit_amd.DropPath) costs: the train step with nothing attached and with DropPath(0.1) attached.

    python tools/droppath_bench.py --out profiles/droppath_bench.log
    python tools/droppath_bench.py --legs eager --full       # per-kernel times of both variants (finds what moved)

Legs (bf16): `eager`, per CONFIG:BATCH of --eager (default base:128) the eager `train_step`; `graphed`, per CONFIG:BATCH of
--graphed (default micro_k:512) the replayed `GraphedTrainStep`; each with a model that has nothing attached and one with
`DropPath(--rate)` attached before the warm-up / capture.

Arithmetic expectation, printed beside every result: the gated row kernels move the bytes of the plain ones plus 4 B per
row (one scalar load), and the draw is one launch of one workgroup that writes 2 * n_layer * B floats - so the step should
cost about one extra launch, microseconds.

Every leg is a child process of its own under `timeout` (this process never opens the GPU; a child that hangs ends there),
and the run stops at the first leg that fails.  Inside a leg the variants alternate, a, b, a, b, ... for --rounds rounds; a
timing is a window of whole calls of at least --window seconds, opened after a warm-up and closed by a device synchronise,
and the figure of a round is window time / calls.  Reported per variant: every round, the median, and the spread
(max - min) / median.  The log (stdout, also written to --out) ends with one DROPPATH_BENCH JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("eager", "graphed")


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


def kernel_times(fn, sync, calls=5):
    """{kernel family: ms per call} from the library's own per-launch profile (events around every launch)."""
    from nvit_amd import ops
    sync()
    ops.prof_collect()
    ops.prof_enable(True)
    try:
        for _ in range(calls):
            fn()
        sync()
    finally:
        ops.prof_enable(False)
    return {k: round(v["ms"] / calls, 4) for k, v in ops.prof_collect().items() if v["launches"]}


def worker(args) -> None:
    sys.path.insert(0, HERE)
    import torch
    from nvit_amd import DropPath
    from nvit_amd.config import named_config
    from nvit_amd.model import ViT
    from nvit_amd.train import GraphedTrainStep, train_step
    from nvit_amd.weights import load_formula_weights
    if not torch.cuda.is_available():
        raise SystemExit("droppath_bench: no GPU (a timing needs the MI355X; there is no fallback)")
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    leg = args.worker
    result = {}

    def images(B, side, C=3):
        g = torch.Generator().manual_seed(B + side)
        return torch.randn(B, C, side, side, generator=g).to(dev)

    def model(cfg, with_dp):
        m = ViT(cfg)
        load_formula_weights(m, cfg)
        m = m.to(dev).set_precision(args.precision).train()
        opt = m.configure_optimizers(1e-3, 1e-3, (0.9, 0.95), "cuda")
        dp = DropPath(args.rate).to(dev) if with_dp else None
        m.attach_drop_path(dp)
        return m, opt, dp

    for spec in (args.graphed if leg == "graphed" else args.eager):
        name, B = spec.split(":")
        B = int(B)
        cfg = named_config(name)
        X, y = images(B, cfg.image_size, cfg.channels), (torch.arange(B) % cfg.num_classes).to(dev)
        (mp, op_, _), (md, od, dp) = model(cfg, False), model(cfg, True)
        if leg == "graphed":
            plain, dropped = GraphedTrainStep(mp, op_, X, y), GraphedTrainStep(md, od, X, y)
            variants = {"step": lambda: plain(X, y), "step+droppath": lambda: dropped(X, y)}
        else:
            variants = {"step": lambda: train_step(mp, op_, X, y), "step+droppath": lambda: train_step(md, od, X, y)}
        r = alternate(variants, args, sync)
        r["droppath_cost_rel"] = round(r["step+droppath"]["median_ms"] / r["step"]["median_ms"] - 1.0, 5)
        r["droppath_cost_ms"] = round(r["step+droppath"]["median_ms"] - r["step"]["median_ms"], 5)
        T = (cfg.image_size // cfg.local_patch_size) ** 2
        r["expected"] = {"extra_launches": 1, "gate_table_bytes": 2 * cfg.n_layer * B * 4,
                         "extra_row_kernel_bytes": 4 * cfg.n_layer * B * T * 4,
                         "note": "4 B per row in each of the 4 gated row-kernel launches of a block; about one launch, us"}
        r["draws"] = dp.step
        if args.full and leg == "eager":
            r["kernel_ms"] = {k: kernel_times(fn, sync) for k, fn in variants.items()}
        last = [train_step(mp, op_, X, y)[1], train_step(md, od, X, y)[1]]
        if not all(torch.isfinite(t).all().item() for t in last):
            raise SystemExit("droppath_bench: non-finite loss")
        result[spec] = r
        print(f"{leg} {spec} {args.precision} rate {args.rate}: {json.dumps(r)}", flush=True)
        del variants, mp, md, op_, od, dp
        if leg == "graphed":
            del plain, dropped
        torch.cuda.empty_cache()
    print("DROPPATH_LEG " + json.dumps({leg: result}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--legs", nargs="*", default=list(LEGS), choices=LEGS)
    ap.add_argument("--eager", nargs="*", default=["base:128"], help="CONFIG:BATCH of the eager-step leg")
    ap.add_argument("--graphed", nargs="*", default=["micro_k:512"], help="CONFIG:BATCH of the replayed-step leg")
    ap.add_argument("--rate", type=float, default=0.1, help="drop rate of the last block")
    ap.add_argument("--precision", default="bf16", choices=("bf16", "fp32"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls of every variant ahead of the rounds")
    ap.add_argument("--window", type=float, default=1.0, help="least seconds of a timed window")
    ap.add_argument("--timeout", type=int, default=240, help="time limit of each leg's child process, seconds")
    ap.add_argument("--full", action="store_true", help="eager leg: also the per-kernel-family times of both variants")
    ap.add_argument("--out", default=None, help="also write the log to this file")
    ap.add_argument("--worker", default=None, choices=LEGS, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        worker(args)
        return 0
    result = {"what": "ms per call; per variant alternating rounds, median and (max-min)/median", "window_s": args.window,
              "rounds": args.rounds, "precision": args.precision, "rate": args.rate}
    log, status = "", 0
    for leg in args.legs:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--worker", leg,
               "--precision", args.precision, "--rounds", str(args.rounds), "--warmup", str(args.warmup),
               "--window", str(args.window), "--rate", str(args.rate), "--graphed", *args.graphed, "--eager", *args.eager]
        if args.full:
            cmd.append("--full")
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if not ln.startswith("DROPPATH_LEG ")]
        part = "\n".join(lines) + "\n"
        done = [ln for ln in r.stdout.splitlines() if ln.startswith("DROPPATH_LEG ")]
        if r.returncode or not done:   # the first failure ends the run: nothing more is started on the GPU
            part += f"leg {leg}: exit status {r.returncode}\n{r.stderr[-3000:]}\n"
            status = 1
        else:
            result.update(json.loads(done[-1][len("DROPPATH_LEG "):]))
        print(part, end="", flush=True)
        log += part
        if status:
            break
    if not status:
        tail = "DROPPATH_BENCH " + json.dumps(result) + "\n"
        print(tail, end="", flush=True)
        log += tail
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(log)
    return status


if __name__ == "__main__":
    sys.exit(main())
