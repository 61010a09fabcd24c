#!/usr/bin/env python3
"""Forward-only throughput: images/s and ms per batch of `with torch.no_grad(): model(X)` in eval mode.

    python tools/eval_bench.py --config base --batch 128 --precision bf16
    python tools/eval_bench.py --config base --batch 128 --against ../other_tree --out profiles/x.json
    python tools/eval_bench.py --config micro_k --batch 512 --graph

`--graph` times `nvit_amd.GraphedEval(model, X, y).predict(X)` instead: the forward replayed as a hipGraph.  That is the
forward without the reconstruction head plus a copy of the logits, so its logits sum equals the plain run's while its
work is slightly less than `model(X)`'s; a tree without GraphedEval fails the round.

Only the public API is used, so the same file measures any tree of this project that has been built: `--against DIR`
measures this tree and the one at DIR in alternation (round 1 here, round 1 there, round 2 here, ...), which is how
two versions are compared.  Every round is its own child process under `timeout` (a round that hangs ends there and
nothing further is started); this process never opens the GPU.  A round warms up, then repeats windows of whole batches
of at least --window seconds, each closed by a device synchronise, and reports the fastest window's time per batch.
Prints one JSON object (also written to --out) and exits; non-zero if a round failed.
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
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    from nvit_amd.config import named_config
    from nvit_amd.model import ViT
    from nvit_amd.weights import load_formula_weights, synthetic_batch
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: no GPU (a timing needs the MI355X; there is no fallback)")
    cfg = named_config(args.config)
    m = ViT(cfg)
    load_formula_weights(m, cfg)
    m = m.to("cuda:0").set_precision(args.precision).eval()
    X, y = (t.to("cuda:0") for t in synthetic_batch(cfg, args.batch))
    if args.graph:
        from nvit_amd import GraphedEval
        step = GraphedEval(m, X, y).predict
    else:
        step = lambda x: m(x)[0]
    with torch.no_grad():
        for _ in range(args.warmup):
            logits = step(X)
        torch.cuda.synchronize()
        windows = []
        for _ in range(args.windows):
            n, t0 = 0, time.perf_counter()
            while True:
                logits = step(X)
                n += 1
                if n % 4 == 0 or args.window == 0:
                    torch.cuda.synchronize()
                    if time.perf_counter() - t0 >= args.window:
                        break
            torch.cuda.synchronize()
            windows.append({"batches": n, "seconds": time.perf_counter() - t0})
    if not torch.isfinite(logits).all().item():
        raise SystemExit("eval_bench: non-finite logits")
    ms = min(w["seconds"] / w["batches"] for w in windows) * 1e3
    print("EVAL_BENCH " + json.dumps({
        "ms_per_batch": round(ms, 4), "images_per_s": round(args.batch / ms * 1e3, 1), "windows": windows,
        "logits_abs_sum": float(logits.double().abs().sum().item()),
        "peak_mem_bytes": torch.cuda.max_memory_allocated()}), flush=True)


def run_round(args, tree: str) -> dict:
    cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--worker",
           "--tree", tree, "--config", args.config, "--batch", str(args.batch), "--precision", args.precision,
           "--warmup", str(args.warmup), "--window", str(args.window), "--windows", str(args.windows)]
    if args.graph:
        cmd.append("--graph")
    r = subprocess.run(cmd, capture_output=True, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("EVAL_BENCH ")]
    if r.returncode != 0 or not lines:
        return {"error": f"exit status {r.returncode}", "stderr_tail": r.stderr[-2000:]}
    return json.loads(lines[-1][len("EVAL_BENCH "):])


def summarize(rounds) -> dict:
    ms = [r["ms_per_batch"] for r in rounds]
    med = statistics.median(ms)
    return {"ms_per_batch_rounds": ms, "ms_per_batch_median": med,
            "images_per_s_median": statistics.median(r["images_per_s"] for r in rounds),
            "spread_ms": round(max(ms) - min(ms), 4), "spread_rel": round((max(ms) - min(ms)) / med, 5),
            "logits_abs_sum": rounds[0]["logits_abs_sum"], "peak_mem_bytes": rounds[0]["peak_mem_bytes"]}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="base")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--precision", default="bf16", choices=("bf16", "fp32"))
    ap.add_argument("--rounds", type=int, default=3, help="child processes per tree")
    ap.add_argument("--warmup", type=int, default=3, help="untimed forwards at the start of a round")
    ap.add_argument("--window", type=float, default=1.5, help="least seconds of a timed window")
    ap.add_argument("--windows", type=int, default=3, help="timed windows per round")
    ap.add_argument("--step-timeout", type=int, default=300, help="time limit of one round, seconds")
    ap.add_argument("--graph", action="store_true", help="time GraphedEval.predict (the forward replayed as a hipGraph)")
    ap.add_argument("--against", default=None, help="a second built tree of this project, measured in alternation")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        worker(args)
        return 0
    trees = [("this", HERE)] + ([("against", os.path.abspath(args.against))] if args.against else [])
    rounds = {k: [] for k, _ in trees}
    failed = None
    for i in range(args.rounds):
        for k, tree in trees:
            r = run_round(args, tree)
            if "error" in r:   # a round faulted, hung or was refused: nothing further is started on the device
                failed = {"tree": k, "round": i, **r}
                break
            rounds[k].append(r)
        if failed:
            break
    out = {"what": "forward-only throughput: eval(), torch.no_grad(), model(X); ms per batch = fastest window of a round",
           "graph": args.graph, "config": args.config, "batch": args.batch, "precision": args.precision, "window_s": args.window,
           "windows_per_round": args.windows, "warmup": args.warmup}
    for k, _ in trees:
        if rounds[k]:
            out[k] = summarize(rounds[k])
    if args.against and not failed:
        a, b = out["this"], out["against"]
        out["this_over_against_time"] = round(a["ms_per_batch_median"] / b["ms_per_batch_median"], 5)
        out["same_logits"] = a["logits_abs_sum"] == b["logits_abs_sum"]
    if failed:
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
