#!/usr/bin/env python3
"""What running at another image size costs (ViT.set_dynamic_img_size / nvit_pos_resample_fwd, _bwd).

    python tools/resize_bench.py --out profiles/resize_bench.log
    python tools/resize_bench.py --legs ab --parent ../parent --out profiles/resize_bench.log

Legs (bf16):
  `resample`  the resample pair alone at --resample C:G:G2 (default 768:28:36, Base at 224 -> 288): forward and backward of
              both tables in one launch each, as calls of the Python wrapper.  Arithmetic expectation, printed beside the
              result: two tables x G2^2 x C x 4 B written (8 MB at the default) is a few microseconds of HBM time, so the
              figure is launch latency, not bandwidth.
  `eager`     per CONFIG:BATCH of --eager (default base:128) the eager `train_step` at the native size with the flag off, at
              the native size with the flag on (the same launches), and at --size (default 288) with the flag on.  A
              measurement: the larger image has (size / native)^2 as many tokens, attention that squared; no claim is made
              about the ratio.
  `ab`        with --parent DIR (the parent commit, checked out and built): tools/ema_ab.sh - bench.py --config base and
              --config micro_k --batch 512 --graph, parent and tree alternating, the --dump-outputs files compared byte for
              byte - logged under this feature's name.  Skipped without --parent.

Every leg is a child process of its own under `timeout` (this process never opens the GPU; a child that hangs ends there),
and the run stops at the first leg that fails.  Inside a leg the variants alternate for --rounds rounds; a timing is a
window of whole calls of at least --window seconds, opened after a warm-up and closed by a device synchronise.  Reported
per variant: every round, the median, and the spread (max - min) / median.  The log (stdout, also written to --out) ends
with one RESIZE_BENCH JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("resample", "eager", "ab")


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
    from nvit_amd.config import named_config
    from nvit_amd.model import ViT
    from nvit_amd.train import train_step
    from nvit_amd.weights import load_formula_weights
    if not torch.cuda.is_available():
        raise SystemExit("resize_bench: no GPU (a timing needs the MI355X; there is no fallback)")
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    leg = args.worker
    result = {}

    if leg == "resample":
        for spec in args.resample:
            C, g, g2 = (int(v) for v in spec.split(":"))
            p0, p1 = torch.randn(g * g, C, device=dev), torch.randn(g * g, C, device=dev)
            d0, d1 = torch.randn(g2 * g2, C, device=dev), torch.randn(g2 * g2, C, device=dev)
            r = alternate({"fwd_pair": lambda: ops.pos_resample_fwd(p0, p1, g, g2),
                           "bwd_pair": lambda: ops.pos_resample_bwd(d0, d1, g, g2),
                           "fwd_one": lambda: ops.pos_resample_fwd(p0, None, g, g2)}, args, sync)
            r["bytes_written"] = {"fwd_pair": 2 * g2 * g2 * C * 4, "bwd_pair": 2 * g * g * C * 4}
            r["note"] = ("timed as calls of the Python wrapper, allocation of the outputs included: launch latency, not "
                         "bandwidth")
            result[spec] = r
            print(f"resample C:g:g2 {spec}: {json.dumps(r)}", flush=True)
        print("RESIZE_LEG " + json.dumps({leg: result}), flush=True)
        return

    def images(B, side, C=3):
        g = torch.Generator().manual_seed(B + side)
        return torch.randn(B, C, side, side, generator=g).to(dev)

    def model(cfg, flag):
        m = ViT(cfg)
        load_formula_weights(m, cfg)
        m = m.to(dev).set_precision(args.precision).train().set_dynamic_img_size(flag)
        return m, m.configure_optimizers(1e-3, 1e-3, (0.9, 0.95), "cuda")

    for spec in args.eager:
        name, B = spec.split(":")
        B = int(B)
        cfg = named_config(name)
        S, P = cfg.image_size, cfg.local_patch_size
        y = (torch.arange(B) % cfg.num_classes).to(dev)
        Xn, Xs = images(B, S, cfg.channels), images(B, args.size, cfg.channels)
        built = {f"{S} flag off": (model(cfg, False), Xn), f"{S} flag on": (model(cfg, True), Xn),
                 f"{args.size} flag on": (model(cfg, True), Xs)}
        variants = {k: (lambda m=m, o=o, X=X: train_step(m, o, X, y)) for k, ((m, o), X) in built.items()}
        r = alternate(variants, args, sync)
        for k, ((m, o), X) in built.items():
            r[k]["tokens"] = (X.shape[-1] // P) ** 2
            r[k]["images_per_s"] = round(B / (r[k]["median_ms"] * 1e-3), 1)
            r[k]["vs_native_flag_off"] = round(r[k]["median_ms"] / r[f"{S} flag off"]["median_ms"], 4)
        last = [fn()[1] for fn in variants.values()]
        if not all(torch.isfinite(t).all().item() for t in last):
            raise SystemExit("resize_bench: non-finite loss")
        result[spec] = r
        print(f"eager {spec} {args.precision}: {json.dumps(r)}", flush=True)
        del variants, built
        torch.cuda.empty_cache()
    print("RESIZE_LEG " + json.dumps({leg: result}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--legs", nargs="*", default=list(LEGS), choices=LEGS)
    ap.add_argument("--resample", nargs="*", default=["768:28:36"], help="C:G:G2 of the resample leg")
    ap.add_argument("--eager", nargs="*", default=["base:128"], help="CONFIG:BATCH of the eager-step leg")
    ap.add_argument("--size", type=int, default=288, help="the other image size of the eager-step leg")
    ap.add_argument("--parent", default=None, help="ab leg: the parent commit, checked out and built")
    ap.add_argument("--precision", default="bf16", choices=("bf16", "fp32"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls of every variant ahead of the rounds")
    ap.add_argument("--window", type=float, default=1.0, help="least seconds of a timed window")
    ap.add_argument("--timeout", type=int, default=300, help="time limit of each leg's child process, seconds")
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
        if leg == "ab":
            if not args.parent:
                part = "leg ab: skipped (no --parent)\n"
                print(part, end="", flush=True)
                log += part
                continue
            ab_log = os.path.join(HERE, "profiles", "resize_ab_bench.log")
            r = subprocess.run(["bash", os.path.join(HERE, "tools", "ema_ab.sh"), os.path.abspath(args.parent), ab_log],
                               capture_output=True, text=True, env=dict(os.environ, ROUNDS=str(args.rounds)))
            part = r.stdout
            if r.returncode:
                part += f"leg ab: exit status {r.returncode}\n{r.stderr[-3000:]}\n"
                status = 1
            else:
                result["ab"] = [ln for ln in r.stdout.splitlines() if "median ms/step" in ln or "--dump-outputs" in ln]
        else:
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--worker", leg,
                   "--precision", args.precision, "--rounds", str(args.rounds), "--warmup", str(args.warmup),
                   "--window", str(args.window), "--resample", *args.resample, "--eager", *args.eager,
                   "--size", str(args.size)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            lines = [ln for ln in r.stdout.splitlines() if not ln.startswith("RESIZE_LEG ")]
            part = "\n".join(lines) + "\n"
            done = [ln for ln in r.stdout.splitlines() if ln.startswith("RESIZE_LEG ")]
            if r.returncode or not done:   # the first failure ends the run: nothing more is started on the GPU
                part += f"leg {leg}: exit status {r.returncode}\n{r.stderr[-3000:]}\n"
                status = 1
            else:
                result.update(json.loads(done[-1][len("RESIZE_LEG "):]))
        print(part, end="", flush=True)
        log += part
        if status:
            break
    if not status:
        tail = "RESIZE_BENCH " + json.dumps(result) + "\n"
        print(tail, end="", flush=True)
        log += tail
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(log)
    return status


if __name__ == "__main__":
    sys.exit(main())
