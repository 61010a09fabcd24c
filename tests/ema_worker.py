"""A run that never constructs a ModelEma, for tests/test_gpu_ema.py: K train steps of micro_k, eager and replayed, with
what they leave behind.  As a program (a fresh process: nvit_amd.ema is never imported) it writes that to an .npz; the
test imports `run` and compares its own runs - no EMA attached, and one attached and detached again - with the file."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

K = 4
NAME, PRECISION, BATCH = "micro_k", "bf16", 8


def build(cfg, precision):
    import torch  # noqa: F401
    from nvit_amd.model import ViT
    from nvit_amd.train import normalize_matrices
    from nvit_amd.weights import formula_state_dict
    m = ViT(cfg)
    res = m.load_state_dict(formula_state_dict(cfg), strict=False)
    assert not res.unexpected_keys and all(k.endswith((".locations", ".offsets")) for k in res.missing_keys)
    m = m.to("cuda:0").set_precision(precision).train()
    normalize_matrices(m)
    return m


def run(before_steps=None):
    """{name: numpy array}: the logits of K eager steps and of 2 replays after them, then weights and moments.
    before_steps(model, optimizer), if given, runs once the optimizer exists."""
    import torch
    from nvit_amd.config import named_config
    from nvit_amd.train import GraphedTrainStep, train_step
    from nvit_amd.weights import synthetic_batch
    cfg = named_config(NAME)
    data = [tuple(t.cuda() for t in synthetic_batch(cfg, BATCH, seed=s)) for s in (1234, 77, 5)]
    m = build(cfg, PRECISION)
    opt = m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    if before_steps is not None:
        before_steps(m, opt)
    out = {}
    for k in range(K):
        logits, loss, _, gnorm = train_step(m, opt, *data[k % 3])
        out[f"logits{k}"], out[f"loss{k}"], out[f"gnorm{k}"] = logits, loss, gnorm
    g = GraphedTrainStep(m, opt, *data[0], warmup=1)
    for k in range(2):
        logits, loss, _, gnorm = g(*data[(k + 1) % 3])
        out[f"rlogits{k}"], out[f"rloss{k}"], out[f"rgnorm{k}"] = logits.clone(), loss.clone(), gnorm.clone()
    for n, p in m.named_parameters():
        out["p." + n] = p.detach()
        if p in opt.state:
            out["m." + n], out["v." + n] = opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]
    out["steps"] = torch.tensor(float(opt.state_dict()["state"][0]["step"]))
    return {k: v.detach().float().cpu().numpy() for k, v in out.items()}


if __name__ == "__main__":
    import numpy as np
    res = run()
    assert "nvit_amd.ema" not in sys.modules
    np.savez(sys.argv[1], **res)
    print("ema_worker: wrote", len(res), "arrays")
