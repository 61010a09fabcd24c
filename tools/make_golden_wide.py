"""Golden vectors of the wide nViT configs (n_embd 1280 and 2048) - runs ONLY where the reference is importable.

Same procedure as oracle/make_golden.py for the BASELINE sizes, whose recorders this tool calls: the real reference model
is imported on the CPU (with an empty `flash_attn` stub), the closed-form formula weights (nvit_amd/weights.py) are loaded
through `load_state_dict` and renormalised, and small records are written to tests/golden/<config>_b<batch>.npz.  Nothing
of the reference travels; only these numbers do.

Recorded per case: the sorted state_dict names and shapes of the formula weights; in the renormalised state the fp32
logits, loss, aux losses, per-parameter gradient norms and the first 8 gradient values, the clipped global gradient norm,
and after one step (clip 1.0, AdamW lr 1e-3, wd 0.1, betas 0.9/0.95, then normalize_matrices) the step-1 logits and the
leading values of h[0].query.weight and h[-1].mlp_c_proj.weight; plus the reference's own bf16 path
(`torch.autocast("cpu", bfloat16)` around the forward) as logits next to its fp32 logits.  Row and column norms are not
recorded: they are 1 by construction.

Usage:  python tools/make_golden_wide.py
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _REPO)

import numpy as np
import torch

from oracle import make_golden as G   # imports the reference (flash_attn stubbed)

from nvit_amd.config import named_config
from nvit_amd.weights import formula_state_dict

CASES = [("wide", 2), ("wide2k", 2), ("wide_k", 2)]


def main() -> None:
    torch.set_num_threads(int(os.environ.get("GOLDEN_THREADS", "8")))
    os.makedirs(G.OUT, exist_ok=True)
    for name, batch in CASES:
        sd = formula_state_dict(named_config(name))
        names = sorted(sd)
        rec = {"sd_names": np.array(names),
               "sd_shapes": np.array(["x".join(str(v) for v in sd[n].shape) for n in names])}
        rec.update(G.one_case(name, batch, True))
        rec.update(G.autocast_case(name, batch))
        path = os.path.join(G.OUT, f"{name}_b{batch}.npz")
        np.savez_compressed(path, **rec)
        print(path, os.path.getsize(path), "bytes; loss %.6f loss1 %.6f gnorm %.6f; autocast max|d| %.3e" %
              (rec["loss"], rec["loss1"], rec["gnorm"], rec["max_abs_dev"]), flush=True)


if __name__ == "__main__":
    main()
