#!/usr/bin/env python3
"""What evaluation's on-device Resize + CenterCrop costs: its two launches alone, next to the training crop followed by
the normalise, and `validate` from stored uint8 data next to `validate` from ready fp32 tensors.

    python tools/center_crop_bench.py --out profiles/center_crop_bench.log
    python tools/center_crop_bench.py --crops 512x40x32 --validate micro_k:512        # a subset

Transform leg, per BxSRCxSIZE (default 128x256x224 and 512x40x32, three channels), for each filter:
`ResizeCenterCrop(SIZE)(u8)` = the two launches with the fp32 output, the same with the uint8 output, and
`normalize_images(rrc.apply(u8, table))` = RandomResizedCrop's two launches on one drawn table plus the normalise's one;
with the bytes the transform has to move (the window's share of the source read once, the fp32 output written once)
and the time they take at the 5.7 TB/s that the row kernels reach: the bar to discuss, not a pass mark.  Validate leg
(bf16), per CONFIG:BATCH
(default base:128): `validate` over --batches batches of fp32 tensors against `validate` over the same number of
`rcc.batch(u8)` from a source of 8/7 the side (256 at 224).

One child process under `timeout` does all of it (this process never opens the GPU; a child that hangs ends there).
Inside it the variants of a leg alternate, a, b, a, b, ... for --rounds rounds; a timing is a window of whole calls of
at least --window seconds, opened after a warm-up and closed by a device synchronise, and the figure of a round is
window time / calls.  Reported per variant: every round, the median, and the spread (max - min) / median.  The log
(stdout, also written to --out) ends with one CENTER_CROP_BENCH JSON line.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from crop_bench import ROW_KERNEL_TBS, alternate  # noqa: E402  (the window and the alternation are crop_bench's)


def worker(args) -> None:
    sys.path.insert(0, HERE)
    import torch
    from nvit_amd import ops
    from nvit_amd.config import named_config
    from nvit_amd.crop import RandomResizedCrop, ResizeCenterCrop
    from nvit_amd.evaluate import validate
    from nvit_amd.model import ViT
    from nvit_amd.weights import load_formula_weights
    if not torch.cuda.is_available():
        raise SystemExit("center_crop_bench: no GPU (a timing needs the MI355X; there is no fallback)")
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    result = {"what": "ms per call; per variant alternating rounds, median and (max-min)/median", "window_s": args.window,
              "rounds": args.rounds, "precision": args.precision, "transform": {}, "validate": {}}

    def bytes_u8(B, side, C=3, seed=0):
        g = torch.Generator().manual_seed(B + side + seed)
        return torch.randint(0, 256, (B, side, side, C), generator=g, dtype=torch.uint8).to(dev)

    for spec in args.crops:
        B, src, size = (int(v) for v in spec.split("x"))
        u8 = bytes_u8(B, src)
        variants = {}
        for f in ("bilinear", "bicubic"):
            rcc = ResizeCenterCrop(size, interpolation=f)
            rrc = RandomResizedCrop(size, interpolation=f, seed=1).to(dev)
            table = rrc.draw(B, src, src)
            variants[f"center fp32 {f}"] = lambda rcc=rcc: rcc(u8)
            variants[f"center uint8 {f}"] = lambda rcc=rcc: rcc(u8, return_u8=True)
            variants[f"rrc.apply + normalize {f}"] = lambda rrc=rrc, table=table: ops.normalize_images(rrc.apply(u8, table))
        r = alternate(variants, args, sync)
        H2, W2, top, _ = ResizeCenterCrop(size).geometry(src, src)
        moved = B * 3 * (src * src * size * size // (H2 * W2) + 4 * size * size)   # the window's share of the source + fp32 out
        r["geometry"] = [H2, W2, top]
        r["bytes_MB"] = round(moved / 1e6, 3)
        r["bytes_at_row_kernel_rate_ms"] = round(moved / (ROW_KERNEL_TBS * 1e12) * 1e3, 5)
        result["transform"][spec] = r
        print(f"transform {spec}x3: {json.dumps(r)}", flush=True)

    for spec in args.validate:
        name, B = spec.split(":")
        B = int(B)
        cfg = named_config(name)
        side = cfg.image_size
        src = 256 if side == 224 else side * 8 // 7
        m = ViT(cfg)
        load_formula_weights(m, cfg)
        m = m.to(dev).set_precision(args.precision)
        rcc = ResizeCenterCrop(side, interpolation="bicubic")
        y = (torch.arange(B) % cfg.num_classes).to(dev)
        stored = [bytes_u8(B, src, cfg.channels, seed=k) for k in range(args.batches)]
        tensors = [(rcc(u), y) for u in stored]
        r = alternate({"validate fp32 tensors": lambda: validate(m, tensors),
                       "validate rcc.batch(u8)": lambda: validate(m, [(rcc.batch(u), y) for u in stored])}, args, sync)
        if validate(m, tensors) != validate(m, [(rcc.batch(u), y) for u in stored]):
            raise SystemExit("center_crop_bench: the two routes disagree")
        r["batches_per_call"] = args.batches
        r["transform_cost_rel"] = round(r["validate rcc.batch(u8)"]["median_ms"] / r["validate fp32 tensors"]["median_ms"] - 1.0, 5)
        r["source"] = f"{src}x{src}x{cfg.channels} uint8"
        result["validate"][spec] = r
        print(f"validate {spec} {args.precision}: {json.dumps(r)}", flush=True)
        del m, tensors, stored
        torch.cuda.empty_cache()
    print("CENTER_CROP_BENCH " + json.dumps(result), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--crops", nargs="*", default=["128x256x224", "512x40x32"], help="BxSRCxSIZE of the transform leg")
    ap.add_argument("--validate", nargs="*", default=["base:128"], help="CONFIG:BATCH of the validate leg")
    ap.add_argument("--batches", type=int, default=4, help="batches per validate call")
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
           "--window", str(args.window), "--batches", str(args.batches), "--crops", *args.crops, "--validate", *args.validate]
    r = subprocess.run(cmd, capture_output=True, text=True)
    log = r.stdout + (f"\nexit status {r.returncode}\n{r.stderr[-3000:]}" if r.returncode else "")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(log)
    print(log, end="")
    return 0 if r.returncode == 0 and "CENTER_CROP_BENCH " in r.stdout else 1


if __name__ == "__main__":
    sys.exit(main())
