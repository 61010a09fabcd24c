"""Stand-alone nvit_renorm_weights (Trainer.normalize_matrices as one launch) and the fused optimizer step
(nvit_grad_sqnorm + nvit_adamw_renorm: clip + AdamW + renorm), warm, on the block weight sets of Base, Large, a
Huge-sized model (n_embd 1280, 32 layers) and n_embd 2048 (8 layers).  Both are HBM-bound and move the same bytes per
element at every width (renorm 8 B: one read + one write; optimizer step 28 B: p, g, m, v read, p, m, v written, plus
4 B for the gradient-norm pass), so the yardstick for the widths over 1152 is the TB/s of the Large set in the same process."""
import os, sys, types
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from nvit_amd import ops
from nvit_amd.optim import FusedAdamW
dev = torch.device("cuda:0")


def timed(fn, warm=3, reps=10):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


SETS = (("base", 768, 12), ("large", 1024, 24), ("huge", 1280, 32), ("2048", 2048, 8))
for name, C, L in [s for s in SETS if not sys.argv[1:] or s[0] in sys.argv[1:]]:   # usage: renorm_bench.py [set ...]
    mats = []
    for _ in range(L):
        for shape, dim in (((C, C), 1), ((C, C), 1), ((C, C), 1), ((C, C), 0), ((8 * C, C), 1), ((C, 4 * C), 0)):
            mats.append((torch.randn(*shape, device=dev), dim))
    for sub, sel in (("all", None), ("rows only (dim=1)", 1), ("columns only (dim=0)", 0)):
        ms_ = [m for m in mats if sel is None or m[1] == sel]
        t, it = ops.renorm_table(ms_, dev)
        nn = sum(w.numel() for w, _ in ms_)
        ms = timed(lambda: ops.renorm_weights(t, it))
        print(f"renorm {name:5s} {sub:22s}: {nn * 8 / 1e6:8.1f} MB  {ms * 1e3:7.1f} us  {nn * 8 / ms / 1e9:7.2f} TB/s", flush=True)
    w, d = mats[3]
    assert (w.norm(dim=0) - 1).abs().max().item() < 1e-5 and (mats[0][0].norm(dim=1) - 1).abs().max().item() < 1e-5
    # the fused optimizer step over the same matrices (weights as left by the renorm above, small gradients); the renorm
    # map comes from blocks that hold all of them, whichever subset the optimizer steps
    params = [torch.nn.Parameter(w) for w, _ in mats]
    W = lambda p: types.SimpleNamespace(weight=p)
    blocks = [types.SimpleNamespace(query=W(q), key=W(k), value=W(v), att_c_proj=W(o), c_fc=W(f), mlp_c_proj=W(pr))
              for q, k, v, o, f, pr in (params[6 * l: 6 * l + 6] for l in range(L))]
    model = types.SimpleNamespace(config=types.SimpleNamespace(use_nvit=True), transformer=types.SimpleNamespace(h=blocks))
    for sub, sel in (("all", None), ("rows only (dim=1)", 1), ("columns only (dim=0)", 0)):
        ps = [p for p, (_, dim) in zip(params, mats) if sel is None or dim == sel]
        for p in ps:
            p.grad = torch.randn_like(p) * 1e-3
        opt = FusedAdamW([{"params": ps, "weight_decay": 0.1}], lr=1e-4, betas=(0.9, 0.95))
        nn = sum(p.numel() for p in ps)
        for clip, nb in ((0.0, 28), (1.0, 32)):
            ms = timed(lambda: opt.step_fused(model, clip))
            print(f"adamw+renorm {name:5s} {sub:22s} clip={clip:3.1f}: {nn * nb / 1e6:8.1f} MB  {ms * 1e3:7.1f} us  "
                  f"{nn * nb / ms / 1e9:7.2f} TB/s", flush=True)
        for p in ps:
            p.grad = None
        del opt, ps
    del mats, params, blocks, model
    torch.cuda.empty_cache()
