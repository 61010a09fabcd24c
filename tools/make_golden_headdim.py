"""Golden vectors of the padded-head-dim configs (head dims 72, 80, 88, 104) - runs ONLY where the reference is importable.

Same procedure as tools/make_golden_wide.py: the recorders of oracle/make_golden.py run the real reference model on the
CPU with the closed-form formula weights (nvit_amd/weights.py), renormalised, and small records are written to
tests/golden/<config>_b<batch>.npz.  The plain-ViT case (use_nvit=False) goes through the repaired-reference recorder of
tools/make_golden_vit.py instead: oracle.make_golden.one_case loads the nViT state dict layout only.  Nothing of the
reference travels; only these numbers do.

Recorded per nViT case: what tools/make_golden_wide.py records (state-dict names and shapes, fp32 logits, loss, aux losses,
per-parameter gradient norms and leading values, the clipped norm, step-1 logits and leading weights, and the reference's
own bf16 autocast logits next to its fp32 logits).  Per plain-ViT case: what tools/make_golden_vit.py records.

Usage:  python tools/make_golden_headdim.py
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _REPO)
sys.path.insert(0, os.path.join(_REPO, "tools"))

import numpy as np
import torch

from oracle import make_golden as G   # imports the reference (flash_attn stubbed)
import make_golden_vit as V           # the same reference module, plus the use_nvit=False repair

from nvit_amd.config import named_config
from nvit_amd.weights import formula_state_dict

CASES = [("hd80", 4), ("hd72", 2), ("hd80_k", 2), ("hd104_b", 2)]
VIT_CASES = [("hd88_vit", 2)]


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
    V._repair_q1()
    for name, batch in VIT_CASES:
        rec = V.one_case(name, batch, True)
        path = os.path.join(G.OUT, f"{name}_b{batch}.npz")
        np.savez_compressed(path, **rec)
        d = np.abs(rec["logits_autocast"] - rec["logits"])
        print(path, os.path.getsize(path), "bytes; loss %.6f gnorm %.6f; autocast max|d| %.3e" %
              (rec["loss"], rec["gnorm"], d.max()), flush=True)


if __name__ == "__main__":
    main()
