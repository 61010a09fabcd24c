#!/usr/bin/env python3
"""What the device-resident dataset costs: its two launches alone, and the train step fed three ways.

    python tools/loader_bench.py --out profiles/loader_bench.log
    python tools/loader_bench.py --pipelines 50000:512x32 --graphed micro_k:512 --eager        # a subset

Pipeline leg, per N:BxSIDE (default 50000:512x32 and 2048:128x256, three channels): `ld()` = nvit_loader_draw +
nvit_loader_gather.  Step legs (bf16), the input chain being `AutoAugment.batch(.)` everywhere: per CONFIG:BATCH of --graphed
(default micro_k:512) the replayed `GraphedTrainStep` called with (a) a device uint8 batch and device labels, as today, (b)
a pinned host uint8 batch and pinned host labels that the call copies in - the most a host loader could deliver: no decode,
no shuffle - and (c) `ld.batch()` and None; per CONFIG:BATCH of --eager (default base:128) the eager `train_step` with (a)
and (c).

One child process under `timeout` does all of it (this process never opens the GPU; a child that hangs ends there).
Inside it the variants of a leg alternate, a, b, c, a, b, c, ... for --rounds rounds; a timing is a window of whole calls of
at least --window seconds, opened after a warm-up and closed by a device synchronise, and the figure of a round is
window time / calls.  Reported per variant: every round, the median, and the spread (max - min) / median.  The log
(stdout, also written to --out) ends with one LOADER_BENCH JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
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
    from nvit_amd.augment import AutoAugment
    from nvit_amd.config import named_config
    from nvit_amd.data import DeviceDataset
    from nvit_amd.model import ViT
    from nvit_amd.train import GraphedTrainStep, train_step
    from nvit_amd.weights import load_formula_weights
    if not torch.cuda.is_available():
        raise SystemExit("loader_bench: no GPU (a timing needs the MI355X; there is no fallback)")
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    result = {"what": "ms per call; per variant alternating rounds, median and (max-min)/median", "window_s": args.window,
              "rounds": args.rounds, "precision": args.precision, "pipeline": {}, "graphed": {}, "eager": {}}

    def dataset(N, side, classes, C=3):
        g = torch.Generator().manual_seed(N + side)
        images = torch.randint(0, 256, (N, side, side, C), dtype=torch.uint8, generator=g)
        return DeviceDataset(images, torch.arange(N) % classes).to(dev)

    for spec in args.pipelines:
        N, shape = spec.split(":")
        B, side = (int(v) for v in shape.split("x"))
        ld = dataset(int(N), side, 10).loader(B, seed=1)
        r = alternate({"draw+gather": lambda: ld()}, args, sync)
        r["batch_MB"] = round(B * side * side * 3 / 1e6, 3)
        r["gather_GB_per_s_read_plus_write"] = round(2 * B * side * side * 3 / r["draw+gather"]["median_ms"] / 1e6, 1)
        result["pipeline"][spec] = r
        print(f"pipeline N={N} {shape}x3: {json.dumps(r)}", flush=True)
        del ld
        torch.cuda.empty_cache()

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
            ds = dataset(max(args.images, B), cfg.image_size, cfg.num_classes, cfg.channels)
            u8, y = ds.images[:B].clone(), ds.labels[:B].clone()
            aug_a, aug_c = AutoAugment("cifar10", seed=1).to(dev), AutoAugment("cifar10", seed=1).to(dev)
            ld = ds.loader(B, seed=1)
            xa, xb = aug_a.batch(u8), aug_c.batch(ld.batch())   # both batch objects are built outside the timed calls
            (ma, oa), (mc, oc) = model(cfg), model(cfg)
            if leg == "graphed":
                u8_pin, y_pin = u8.cpu().pin_memory(), y.cpu().pin_memory()
                tensor, loader = GraphedTrainStep(ma, oa, xa, y), GraphedTrainStep(mc, oc, xb, None)
                variants = {"a device tensor": lambda: tensor(u8, y), "b pinned host batch": lambda: tensor(u8_pin, y_pin),
                            "c loader": lambda: loader(xb, None)}
            else:
                variants = {"a device tensor": lambda: train_step(ma, oa, xa, y),
                            "c loader": lambda: train_step(mc, oc, xb, None)}
            r = alternate(variants, args, sync)
            base = r["a device tensor"]["median_ms"]
            for k in variants:
                if k != "a device tensor":
                    r[k]["minus_a_us"] = round((r[k]["median_ms"] - base) * 1e3, 2)
            last = [train_step(ma, oa, xa, y)[1], train_step(mc, oc, xb, None)[1]]
            if not all(torch.isfinite(t).all().item() for t in last):
                raise SystemExit("loader_bench: non-finite loss")
            r["loader_epoch_step"] = [ld.epoch, ld.step]
            result[leg][spec] = r
            print(f"{leg} {spec} {args.precision}: {json.dumps(r)}", flush=True)
            del variants, ma, mc, oa, oc, ds, ld, xa, xb
            if leg == "graphed":
                del tensor, loader
            torch.cuda.empty_cache()
    print("LOADER_BENCH " + json.dumps(result), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pipelines", nargs="*", default=["50000:512x32", "2048:128x256"], help="N:BxSIDE of the pipeline leg")
    ap.add_argument("--graphed", nargs="*", default=["micro_k:512"], help="CONFIG:BATCH of the replayed-step leg")
    ap.add_argument("--eager", nargs="*", default=["base:128"], help="CONFIG:BATCH of the eager-step leg")
    ap.add_argument("--images", type=int, default=2048, help="images of the step legs' dataset (at least the batch)")
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
           "--window", str(args.window), "--images", str(args.images), "--pipelines", *args.pipelines,
           "--graphed", *args.graphed, "--eager", *args.eager]
    with tempfile.TemporaryFile("w+") as errfile:
        child = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=errfile, text=True)
        lines = []
        for line in child.stdout:   # shown as it comes: a leg takes a while
            lines.append(line)
            print(line, end="", flush=True)
        rc = child.wait()
        errfile.seek(0)
        err = errfile.read()
    tail = f"\nexit status {rc}\n{err[-3000:]}" if rc else ""
    print(tail, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("".join(lines) + tail)
    return 0 if rc == 0 and any(ln.startswith("LOADER_BENCH ") for ln in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
