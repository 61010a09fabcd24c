#!/usr/bin/env python3
"""What patch dropout (nvit_amd.PatchDropout) buys: the train step with nothing attached and with PatchDropout(rate) attached.

    python tools/patchdrop_bench.py --out profiles/patchdrop_bench.log
    python tools/patchdrop_bench.py --legs eager --eager base:128 --rates 0.5 --full     # per-kernel-family times

Legs (bf16): `eager`, per CONFIG:BATCH of --eager (default base:128 huge16:64) the eager `train_step`; `graphed`, per
CONFIG:BATCH of --graphed (default tiny:512; the Kohonen configs do not take patch dropout) the replayed
`GraphedTrainStep`; each with a model that has nothing attached (rate 0) and one model per --rates entry with
`PatchDropout(rate)` attached before the warm-up / capture.  `rows`: nvit_rows_gather (both streams, with twins) and
nvit_rows_scatter alone at --rows B:T:C (default 128:784:768) and --rows-rate (default 0.5), in TB/s of algorithmic
bytes.

Arithmetic expectation, printed beside every result: at K of T tokens every GEMM and row kernel behind the gather does K/T
of the work, attention (K/T)^2, the patch embedding and the optimizer stay; the feature itself adds three launches forward
(draw, counter, gather) and one backward (scatter).  Every K-token shape is listed with the route it takes (ops.fusable
decides by the shape): a K-token shape may fall off a fused route that the T-token shape takes.

Every leg is a child process of its own under `timeout` (this process never opens the GPU; a child that hangs ends there),
and the run stops at the first leg that fails.  Inside a leg the variants alternate, a, b, c, a, b, c, ... for --rounds
rounds; a timing is a window of whole calls of at least --window seconds, opened after a warm-up and closed by a device
synchronise, and the figure of a round is window time / calls.  Reported per variant: every round, the median, and the
spread (max - min) / median.  The log (stdout, also written to --out) ends with one PATCHDROP_BENCH JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("eager", "graphed", "rows")


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


def routes(cfg, B, Tk, dt):
    """the shape-dependent route choices of a forward over Tk tokens per sample (model.py: _attn_fwd, _swiglu_fwd/bwd)"""
    from nvit_amd import ops
    C, M = cfg.n_embd, B * Tk
    d = C // cfg.n_head
    qk = (not cfg.flash_attn) and d == 64 and C % 256 == 0
    return {"rows": M, "qkv": "fused" if qk and ops.fusable(dt, M, 3 * C, C) else "split",
            "cross_q": "fused" if qk and ops.fusable(dt, M, C, C) else "split",
            "c_fc_swiglu": "fused" if ops.fusable(dt, M, 8 * C, C) else "gemm+row kernel",
            "c_proj_swiglu_bwd": "fused" if ops.fusable(dt, M, 4 * C, C) else "gemm+row kernel"}


def worker(args) -> None:
    sys.path.insert(0, HERE)
    import torch
    from nvit_amd import PatchDropout, ops
    from nvit_amd._lib import BF16, F32
    from nvit_amd.config import named_config
    from nvit_amd.model import ViT
    from nvit_amd.train import GraphedTrainStep, train_step
    from nvit_amd.weights import load_formula_weights
    if not torch.cuda.is_available():
        raise SystemExit("patchdrop_bench: no GPU (a timing needs the MI355X; there is no fallback)")
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    leg = args.worker
    result = {}
    dt = BF16 if args.precision == "bf16" else F32

    if leg == "rows":
        for spec in args.rows:
            B, T, C = (int(v) for v in spec.split(":"))
            pd = PatchDropout(args.rows_rate).to(dev)
            K = pd.num_keep(T)
            keep, slot = pd.draw(B, T)
            s0, s1 = torch.randn(B * T, C, device=dev), torch.randn(B * T, C, device=dev)
            d0, d1 = torch.randn(B * K, C, device=dev), torch.randn(B * K, C, device=dev)
            r = alternate({"gather": lambda: ops.rows_gather(s0, s1, keep, B, T, lo_dt=BF16),
                           "gather_no_twins": lambda: ops.rows_gather(s0, s1, keep, B, T),
                           "scatter": lambda: ops.rows_scatter(d0, d1, slot, B, K),
                           "draw": lambda: pd.draw(B, T)}, args, sync)
            nbytes = {"gather": 2 * B * K * C * 10, "gather_no_twins": 2 * B * K * C * 8,
                      "scatter": 2 * (B * K * C * 4 + B * T * C * 4)}
            for k, n in nbytes.items():
                r[k]["algorithmic_bytes"] = n
                r[k]["tb_per_s"] = round(n / (r[k]["median_ms"] * 1e-3) / 1e12, 3)
            r["note"] = ("timed as calls of the Python wrapper, allocation of the outputs included; the neighbouring row "
                         "kernels reach 5.2-5.8 TB/s on rows of this width")
            result[spec] = {"K": K, **r}
            print(f"rows {spec} rate {args.rows_rate} K={K}: {json.dumps(result[spec])}", flush=True)
        print("PATCHDROP_LEG " + json.dumps({leg: result}), flush=True)
        return

    def images(B, side, C=3):
        g = torch.Generator().manual_seed(B + side)
        return torch.randn(B, C, side, side, generator=g).to(dev)

    def model(cfg, rate):
        m = ViT(cfg)
        load_formula_weights(m, cfg)
        m = m.to(dev).set_precision(args.precision).train()
        opt = m.configure_optimizers(1e-3, 1e-3, (0.9, 0.95), "cuda")
        pd = PatchDropout(rate).to(dev) if rate > 0 else None
        m.attach_patch_drop(pd)
        return m, opt, pd

    for spec in (args.graphed if leg == "graphed" else args.eager):
        name, B = spec.split(":")
        B = int(B)
        cfg = named_config(name)
        T = (cfg.image_size // cfg.local_patch_size) ** 2
        X, y = images(B, cfg.image_size, cfg.channels), (torch.arange(B) % cfg.num_classes).to(dev)
        built = {f"rate {rate:g}": model(cfg, rate) for rate in [0.0] + [r for r in args.rates if r > 0]}
        if leg == "graphed":
            steps = {k: GraphedTrainStep(m, o, X, y) for k, (m, o, _) in built.items()}
            variants = {k: (lambda s=s: s(X, y)) for k, s in steps.items()}
        else:
            variants = {k: (lambda m=m, o=o: train_step(m, o, X, y)) for k, (m, o, _) in built.items()}
        r = alternate(variants, args, sync)
        base_ms = r["rate 0"]["median_ms"]
        for k, (m, o, pd) in built.items():
            Tk = pd.num_keep(T) if pd is not None else T
            r[k]["tokens"] = Tk
            r[k]["images_per_s"] = round(B / (r[k]["median_ms"] * 1e-3), 1)
            r[k]["speedup_vs_rate_0"] = round(base_ms / r[k]["median_ms"], 4)
            r[k]["routes"] = routes(cfg, B, Tk, dt)
            r[k]["draws"] = pd.step if pd is not None else 0
            r[k]["expected_share"] = {"gemm_and_rows": round(Tk / T, 4), "attention": round((Tk / T) ** 2, 4)}
        if args.full and leg == "eager":
            for k, fn in variants.items():
                r[k]["kernel_ms"] = kernel_times(fn, sync)
        last = [train_step(m, o, X, y)[1] for m, o, _ in built.values()] if leg == "eager" else [s.loss for s in steps.values()]
        if not all(torch.isfinite(t).all().item() for t in last):
            raise SystemExit("patchdrop_bench: non-finite loss")
        result[spec] = r
        print(f"{leg} {spec} {args.precision} T={T}: {json.dumps(r)}", flush=True)
        del variants, built
        if leg == "graphed":
            del steps
        torch.cuda.empty_cache()
    print("PATCHDROP_LEG " + json.dumps({leg: result}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--legs", nargs="*", default=list(LEGS), choices=LEGS)
    ap.add_argument("--eager", nargs="*", default=["base:128", "huge16:64"], help="CONFIG:BATCH of the eager-step leg")
    ap.add_argument("--graphed", nargs="*", default=["tiny:512"], help="CONFIG:BATCH of the replayed-step leg")
    ap.add_argument("--rows", nargs="*", default=["128:784:768"], help="B:T:C of the gather / scatter leg")
    ap.add_argument("--rates", nargs="*", type=float, default=[0.25, 0.5], help="drop rates (rate 0 always runs beside them)")
    ap.add_argument("--rows-rate", type=float, default=0.5, help="drop rate of the gather / scatter leg")
    ap.add_argument("--precision", default="bf16", choices=("bf16", "fp32"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls of every variant ahead of the rounds")
    ap.add_argument("--window", type=float, default=1.0, help="least seconds of a timed window")
    ap.add_argument("--timeout", type=int, default=300, help="time limit of each leg's child process, seconds")
    ap.add_argument("--full", action="store_true", help="eager leg: also the per-kernel-family times of every variant")
    ap.add_argument("--out", default=None, help="also write the log to this file")
    ap.add_argument("--worker", default=None, choices=LEGS, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        worker(args)
        return 0
    result = {"what": "ms per call; per variant alternating rounds, median and (max-min)/median", "window_s": args.window,
              "rounds": args.rounds, "precision": args.precision, "rates": args.rates}
    log, status = "", 0
    for leg in args.legs:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--worker", leg,
               "--precision", args.precision, "--rounds", str(args.rounds), "--warmup", str(args.warmup),
               "--window", str(args.window), "--rates", *[str(r) for r in args.rates], "--graphed", *args.graphed,
               "--eager", *args.eager, "--rows", *args.rows, "--rows-rate", str(args.rows_rate)]
        if args.full:
            cmd.append("--full")
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if not ln.startswith("PATCHDROP_LEG ")]
        part = "\n".join(lines) + "\n"
        done = [ln for ln in r.stdout.splitlines() if ln.startswith("PATCHDROP_LEG ")]
        if r.returncode or not done:   # the first failure ends the run: nothing more is started on the GPU
            part += f"leg {leg}: exit status {r.returncode}\n{r.stderr[-3000:]}\n"
            status = 1
        else:
            result.update(json.loads(done[-1][len("PATCHDROP_LEG "):]))
        print(part, end="", flush=True)
        log += part
        if status:
            break
    if not status:
        tail = "PATCHDROP_BENCH " + json.dumps(result) + "\n"
        print(tail, end="", flush=True)
        log += tail
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(log)
    return status


if __name__ == "__main__":
    sys.exit(main())
