#!/usr/bin/env python3
"""Train-step time with `skip_nonfinite` off and on, measured in alternation (no threshold: a measurement).

    python tools/skip_guard_bench.py --config base --batch 128
    python tools/skip_guard_bench.py --config micro_k --batch 512
    python tools/skip_guard_bench.py --config micro_k --batch 512 --graph --out profiles/x.json

Times `nvit_amd.train.train_step` (or, with --graph, `GraphedTrainStep` replays) on one synthetic batch.  The guarded
step issues nvit_grad_sqnorm, the guarded tick and the guarded update where the clipped step issues the tick,
nvit_grad_sqnorm and the update: the same number of launches, a 1024-thread tick instead of a 1-thread one, and one
flag load per workgroup.  Rounds alternate off, on, off, on, ...; every round is its own child process under `timeout`
(a round that hangs ends there and nothing further is started); this process never opens the GPU.  A round warms up, then
repeats windows of whole steps of at least --window seconds, each closed by a device synchronise, and reports the
fastest window's time per step.  Prints one JSON object (also written to --out); non-zero exit if a round failed.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(args) -> None:
    sys.path.insert(0, HERE)
    import torch
    from nvit_amd.config import named_config
    from nvit_amd.model import ViT
    from nvit_amd.train import GraphedTrainStep, normalize_matrices, train_step
    from nvit_amd.weights import load_formula_weights, synthetic_batch
    if not torch.cuda.is_available():
        raise SystemExit("skip_guard_bench: no GPU (a timing needs the MI355X; there is no fallback)")
    cfg = named_config(args.config)
    m = ViT(cfg)
    load_formula_weights(m, cfg)
    m = m.to("cuda:0").set_precision(args.precision).train()
    normalize_matrices(m)
    opt = m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    X, y = (t.to("cuda:0") for t in synthetic_batch(cfg, args.batch))
    guard = bool(args.guard)
    if args.graph:
        g = GraphedTrainStep(m, opt, X, y, 1.0, warmup=args.warmup, skip_nonfinite=guard)
        step = lambda: g(X, y)
    else:
        step = lambda: train_step(m, opt, X, y, 1.0, skip_nonfinite=guard)
        for _ in range(args.warmup):
            step()
    torch.cuda.synchronize()
    windows = []
    for _ in range(args.windows):
        n, t0 = 0, time.perf_counter()
        while True:
            out = step()
            n += 1
            if n % 4 == 0 or args.window == 0:
                torch.cuda.synchronize()
                if time.perf_counter() - t0 >= args.window:
                    break
        torch.cuda.synchronize()
        windows.append({"steps": n, "seconds": time.perf_counter() - t0})
    loss = float(out[1].item())
    if loss != loss or (guard and opt.skipped_steps() != 0):
        raise SystemExit("skip_guard_bench: the timed steps were not ordinary applied steps")
    ms = min(w["seconds"] / w["steps"] for w in windows) * 1e3
    print("SKIP_GUARD_BENCH " + json.dumps({"ms_per_step": round(ms, 4), "windows": windows, "loss": loss}), flush=True)


def run_round(args, guard: int) -> dict:
    cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--worker",
           "--guard", str(guard), "--config", args.config, "--batch", str(args.batch), "--precision", args.precision,
           "--warmup", str(args.warmup), "--window", str(args.window), "--windows", str(args.windows)]
    if args.graph:
        cmd.append("--graph")
    r = subprocess.run(cmd, capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("SKIP_GUARD_BENCH ")]
    if r.returncode != 0 or not lines:
        return {"error": f"exit status {r.returncode}", "stderr_tail": r.stderr[-2000:]}
    return json.loads(lines[-1][len("SKIP_GUARD_BENCH "):])


def summarize(rounds) -> dict:
    ms = [r["ms_per_step"] for r in rounds]
    med = statistics.median(ms)
    return {"ms_per_step_rounds": ms, "ms_per_step_median": med, "spread_ms": round(max(ms) - min(ms), 4),
            "spread_rel": round((max(ms) - min(ms)) / med, 5)}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="base")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--precision", default="bf16", choices=("bf16", "fp32"))
    ap.add_argument("--rounds", type=int, default=3, help="child processes per setting")
    ap.add_argument("--warmup", type=int, default=3, help="untimed steps at the start of a round")
    ap.add_argument("--window", type=float, default=1.5, help="least seconds of a timed window")
    ap.add_argument("--windows", type=int, default=3, help="timed windows per round")
    ap.add_argument("--step-timeout", type=int, default=300, help="time limit of one round, seconds")
    ap.add_argument("--graph", action="store_true", help="time GraphedTrainStep replays instead of eager steps")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    ap.add_argument("--guard", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        worker(args)
        return 0
    rounds = {"off": [], "on": []}
    failed = None
    for i in range(args.rounds):
        for k, guard in (("off", 0), ("on", 1)):
            r = run_round(args, guard)
            if "error" in r:   # a round faulted, hung or was refused: nothing further is started on the device
                failed = {"skip_nonfinite": k, "round": i, **r}
                break
            rounds[k].append(r)
        if failed:
            break
    out = {"what": "train step time, skip_nonfinite off / on in alternation; ms per step = fastest window of a round",
           "graph": args.graph, "config": args.config, "batch": args.batch, "precision": args.precision,
           "window_s": args.window, "windows_per_round": args.windows, "warmup": args.warmup}
    for k in rounds:
        if rounds[k]:
            out[k] = summarize(rounds[k])
    if not failed:
        out["on_over_off_time"] = round(out["on"]["ms_per_step_median"] / out["off"]["ms_per_step_median"], 5)
    else:
        out["failed"] = failed
    text = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
