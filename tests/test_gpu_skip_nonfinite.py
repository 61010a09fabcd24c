"""GPU: `skip_nonfinite`, the fused step's counterpart of the reference's GradScaler.step (train.py:930-942): an
optimizer step whose gradients hold inf or NaN - or whose squared norm overflows fp32 - is left out on the device.

A skipped step must leave every parameter, both moments and the step counter bit-identical, wherever in the parameter
table the offending element sits (every item kind of the optimizer kernel); an applied step must give the bits of the
unguarded step; and a run that meets one poisoned batch must continue exactly as if that batch had never come, eagerly
and through hipGraph replays, where no host code could notice."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from nvit_amd.config import named_config
from nvit_amd.weights import formula_state_dict, synthetic_batch


def build(cfg, precision):
    from nvit_amd.model import ViT
    from nvit_amd.train import normalize_matrices
    m = ViT(cfg)
    res = m.load_state_dict(formula_state_dict(cfg), strict=False)
    assert not res.unexpected_keys and all(k.endswith((".locations", ".offsets")) for k in res.missing_keys)
    m = m.to("cuda:0").set_precision(precision).train()
    normalize_matrices(m)
    return m


def optimizer(m):
    return m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")


def op_config(name):
    return named_config("wide", n_layer=1) if name == "wide" else named_config(name)


def backward(m, X, y):
    from nvit_amd.train import total_loss
    logits, aux = m(X)
    total_loss(m.config, logits, aux, y).backward()


def table_order(opt):
    """The parameters in the order of the optimizer's device table: group by group, those with a gradient."""
    return [p for g in opt.param_groups for p in g["params"] if p.grad is not None]


def snapshot(opt, params):
    return [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in params]


def assert_untouched(opt, params, snap, what):
    for p, (p0, m0, v0) in zip(params, snap):
        # bit-identical: compare the words (NaN-safe, and -0.0 is not 0.0)
        assert torch.equal(p.detach().view(torch.int32), p0.view(torch.int32)), (what, tuple(p.shape), "param")
        assert torch.equal(opt.state[p]["exp_avg"].view(torch.int32), m0.view(torch.int32)), (what, "exp_avg")
        assert torch.equal(opt.state[p]["exp_avg_sq"].view(torch.int32), v0.view(torch.int32)), (what, "exp_avg_sq")


def steps_in(opt):
    return {int(float(st["step"])) for st in opt.state_dict()["state"].values()}


@pytest.mark.parametrize("name", ["micro", "wide"])
def test_poisoned_gradient_skips_the_step_wherever_it_sits(name):
    """One gradient element overwritten by inf, NaN or 1e30 (finite, but its square overflows fp32), in turn at: the
    first element of the first table entry, the last element of the last one, inside a row-normalised matrix, inside a
    column-normalised matrix (on `wide`, 1280 rows: the tall 16-column slab) and in a 1-D parameter."""
    cfg = op_config(name)
    X, y = (t.cuda() for t in synthetic_batch(cfg, 4))
    m = build(cfg, "bf16")
    opt = optimizer(m)
    backward(m, X, y)
    opt.step_fused(m, 1.0, skip_nonfinite=True)       # an applied step first: the moments are not zero, the count is 1
    opt.zero_grad(set_to_none=True)
    assert opt.skip_state.tolist() == [0.0, 0.0] and steps_in(opt) == {1}
    backward(m, X, y)
    params = table_order(opt)
    blk = m.transformer.h[0]
    rowm, colm = blk.query.weight, blk.att_c_proj.weight
    assert colm.shape[0] == cfg.n_embd and (name != "wide" or colm.shape[0] == 1280)
    vec = next(p for p in params if p.dim() == 1 and p.numel() > 1)
    spots = [("first of first", params[0], 0), ("last of last", params[-1], params[-1].numel() - 1),
             ("row-normalised", rowm, rowm.numel() // 2 + 3), ("column-normalised", colm, colm.numel() - colm.shape[1] // 2),
             ("1-D", vec, vec.numel() - 1)]
    assert all(any(p is q for q in params) for _, p, _ in spots)
    snap = snapshot(opt, params)
    k = 0
    for clip in (1.0, 0.0):
        for where, p, idx in spots:
            for bad in (float("inf"), float("nan"), 1e30):
                what = (name, clip, where, bad)
                g = p.grad.view(-1)
                keep = g[idx].clone()
                assert math.isfinite(keep.item()), what
                g[idx] = bad
                gnorm = opt.step_fused(m, clip, skip_nonfinite=True)
                k += 1
                assert gnorm is not None and not math.isfinite(gnorm.item()), (what, gnorm)
                assert opt.skip_state.tolist() == [1.0, float(k)], (what, opt.skip_state.tolist())
                assert_untouched(opt, params, snap, what)
                assert steps_in(opt) == {1}, (what, steps_in(opt))
                g[idx] = keep
    assert opt.skipped_steps() == k == 30
    # ... and the guard lets go again: the restored gradients give the step of an unguarded twin
    gnorm = opt.step_fused(m, 1.0, skip_nonfinite=True)
    assert math.isfinite(gnorm.item()) and opt.skip_state.tolist() == [0.0, float(k)] and steps_in(opt) == {2}
    twin = build(cfg, "bf16")
    topt = optimizer(twin)
    for _ in range(2):
        backward(twin, X, y)
        tnorm = topt.step_fused(twin, 1.0)
        topt.zero_grad(set_to_none=True)
    assert torch.equal(gnorm, tnorm)
    for p, q in zip(m.parameters(), twin.parameters()):
        assert torch.equal(p, q)


@pytest.mark.parametrize("name", ["micro", "wide"])
@pytest.mark.parametrize("clip", [1e-3, 1e6, 0.0])     # clipping active, inactive (the norm is far below), off
def test_applied_steps_are_those_of_the_unguarded_step(clip, name):
    cfg = op_config(name)
    X, y = (t.cuda() for t in synthetic_batch(cfg, 4))
    ma, mb = build(cfg, "bf16"), build(cfg, "bf16")
    oa, ob = optimizer(ma), optimizer(mb)
    for step in range(2):
        backward(ma, X, y)
        backward(mb, X, y)
        ga = oa.step_fused(ma, clip, skip_nonfinite=True)
        gb = ob.step_fused(mb, clip, skip_nonfinite=False)
        assert ga is not None and math.isfinite(ga.item())      # the norm is reported whenever the guard is on
        if clip > 0.0:
            assert torch.equal(ga, gb), (ga.item(), gb.item())
            assert (ga.item() > clip) == (clip == 1e-3), (ga.item(), clip)
        else:
            assert gb is None
        for pa, pb in zip(table_order(oa), table_order(ob)):
            assert torch.equal(pa, pb), (step, tuple(pa.shape))
            for key in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(oa.state[pa][key], ob.state[pb][key]), (step, key, tuple(pa.shape))
        oa.zero_grad(set_to_none=True)
        ob.zero_grad(set_to_none=True)
    assert oa.skip_state.tolist() == [0.0, 0.0] and oa.skipped_steps() == 0
    assert steps_in(oa) == steps_in(ob) == {2}


def _nan_pixel(X, row):
    X = X.clone()
    X[row, 1, 5, 7] = float("nan")
    return X


def _same_run(ma, mb, oa, ob):
    n = 0
    for (name, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.isfinite(pa).all(), name
        assert torch.equal(pa, pb), name
        if pa in oa.state:
            n += 1
            for key in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(oa.state[pa][key], ob.state[pb][key]), (name, key)
    assert n > 10
    assert steps_in(oa) == steps_in(ob) == {2}, (steps_in(oa), steps_in(ob))
    assert oa.skipped_steps() == 1 and oa.skip_state.tolist() == [0.0, 1.0]


def _recovery(precision, graphed, N):
    """Model A: a clean step, a step on a batch with one NaN pixel (in the LAST micro-batch), a clean step, all guarded.
    Model B: the two clean steps, unguarded.  A must be B."""
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = named_config("mini")       # no Kohonen head: no index is derived from a NaN distance
    rows = 4 * N
    (X0, y0), (X1, y1), (X2, y2) = [tuple(t.cuda() for t in synthetic_batch(cfg, rows, seed=s)) for s in (1234, 77, 5)]
    X1 = _nan_pixel(X1, rows - 1)
    ma, mb = build(cfg, precision), build(cfg, precision)
    oa, ob = optimizer(ma), optimizer(mb)
    kw = dict(accumulation_steps=N)
    if graphed:
        g = GraphedTrainStep(ma, oa, X0, y0, warmup=1, skip_nonfinite=True, **kw)     # its warm-up is the first step
        bad = g(X1, y1)
        bad = [bad[1].clone(), bad[3].clone()]
        good = g(X2, y2)
    else:
        train_step(ma, oa, X0, y0, skip_nonfinite=True, **kw)
        bad = train_step(ma, oa, X1, y1, skip_nonfinite=True, **kw)
        bad = [bad[1], bad[3]]
        good = train_step(ma, oa, X2, y2, skip_nonfinite=True, **kw)
    assert all(not math.isfinite(t.item()) for t in bad), bad          # loss and norm of the poisoned step
    train_step(mb, ob, X0, y0, **kw)
    ref = train_step(mb, ob, X2, y2, **kw)
    assert torch.equal(good[0], ref[0]) and torch.equal(good[1], ref[1]) and torch.equal(good[3], ref[3])
    _same_run(ma, mb, oa, ob)
    assert (ma.step, mb.step) == (3 * N, 2 * N)


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_run_recovers_from_a_nan_batch(precision, graphed):
    _recovery(precision, graphed, 1)


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
def test_nan_in_the_second_micro_batch_skips_the_whole_accumulated_step(graphed):
    _recovery("bf16", graphed, 2)


def test_without_the_guard_the_same_batch_destroys_the_weights():
    """The control of the recovery tests: the poisoned batch does reach the optimizer."""
    from nvit_amd.train import train_step
    cfg = named_config("mini")
    (X0, y0), (X1, y1) = [tuple(t.cuda() for t in synthetic_batch(cfg, 4, seed=s)) for s in (1234, 77)]
    m = build(cfg, "bf16")
    opt = optimizer(m)
    train_step(m, opt, X0, y0)
    _, loss, _, gnorm = train_step(m, opt, _nan_pixel(X1, 3), y1)
    assert not math.isfinite(loss.item()) and not math.isfinite(gnorm.item())
    assert torch.isnan(m.transformer.h[0].query.weight).any() and torch.isnan(m.mlp_head[1].weight).any()
    assert steps_in(opt) == {2}
