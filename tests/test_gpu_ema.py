"""GPU: ModelEma on real train steps (micro_k, mini, micro_vit at batch 8; bf16 and fp32).

The shadow against the fp64 recurrence over the weights the steps left; replayed steps against eager ones bit for bit
(the EMA is captured with the step); a step that skip_nonfinite leaves out; the re-normalised module of an nViT and the
shared-storage module of a plain ViT; evaluation through the module; attach / detach; the checkpoint round trip."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ema_ref
import ema_worker
import optim_check as oc
from ema_worker import build
from nvit_amd.config import named_config
from nvit_amd.weights import synthetic_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEDULE = dict(kohonen_alpha=0.5, kohonen_scheduler_enabled=True, kohonen_scheduler_warmup_steps=3,
                kohonen_scheduler_decay_steps=7, kohonen_scheduler_min_lr=0.05)   # of test_gpu_graph_kohonen.py
B = 8


def optimizer(m):
    return m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")


def batches(cfg, rows=B):
    return [tuple(t.cuda() for t in synthetic_batch(cfg, rows, seed=s)) for s in (1234, 77, 5)]


def with_ema(cfg, precision, **kw):
    from nvit_amd import ModelEma
    m = build(cfg, precision)
    opt = optimizer(m)
    ema = ModelEma(m, **kw)
    opt.attach_ema(ema)
    return m, opt, ema


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


def assert_same_shadow(a, b, what):
    sa, sb = a.shadow, b.shadow
    assert list(sa) == list(sb), what
    for n in sa:
        assert same_bits(sa[n], sb[n]), (what, n, (sa[n] - sb[n]).abs().max().item())


def assert_same_weights(ma, mb, what):
    for (n, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert same_bits(pa, pb), (what, n)


def snapshot(ema):
    return {n: t.clone() for n, t in ema.shadow.items()}


def third_model(ema, cfg, precision):
    """A ViT loaded from the saved shadow and re-normalised by the stand-alone kernel: what ema.module must be"""
    from nvit_amd.model import ViT
    from nvit_amd.train import normalize_matrices
    m = ViT(cfg)
    res = m.load_state_dict({n: t.cpu() for n, t in ema.state_dict()["shadow"].items()}, strict=False)
    assert not res.unexpected_keys and all(k.endswith((".locations", ".offsets")) for k in res.missing_keys)
    m = m.to("cuda:0").set_precision(precision).eval()
    normalize_matrices(m)
    return m


# --------------------------------------------------------------------------------------------- 1. the recurrence
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["micro_k", "mini", "micro_vit"])
def test_shadow_follows_the_fp64_recurrence(name, precision):
    from nvit_amd.train import train_step
    K = 5
    cfg = named_config(name)
    data = batches(cfg)
    m, opt, ema = with_ema(cfg, precision, warmup=True)
    names = [n for n, p in m.named_parameters()]
    assert list(ema.shadow) == names and ("local_kohonen.nodes" in names) == cfg.use_kohonen
    for n, p in m.named_parameters():      # the shadow starts as a copy of the weights
        assert same_bits(ema.shadow[n], p), n
    assert ema.updates == 0
    e0 = {n: t.cpu().numpy() for n, t in ema.shadow.items()}
    weights, omds = [], []
    for k in range(K):
        train_step(m, opt, *data[k % 3])
        weights.append({n: p.detach().cpu().numpy() for n, p in m.named_parameters()})
        st = ema.state.cpu().numpy()
        assert st[0] == k + 1 and st[1].tobytes() == ema_ref.omd_at(k, 0.9998, True).tobytes(), (k, st)
        omds.append(st[1])
    assert ema.updates == K
    worst, moved = 0.0, 0
    for n, got in ema.state_dict()["shadow"].items():
        got = got.cpu().numpy()
        ws = [w[n] for w in weights]
        ref = ema_ref.recurrence(e0[n], ws, omds)
        amp = np.max(np.abs(np.stack([e0[n]] + ws + [got])), axis=0).astype(np.float64)
        err, bound = np.abs(got.astype(np.float64) - ref), K * 2.0 ** -22 * amp
        assert (err <= bound).all(), (n, float(err.max()), int(np.argmax(err - bound)))
        nz = bound > 0
        worst = max(worst, float((err[nz] / bound[nz]).max()) if nz.any() else 0.0)
        moved += int(not np.array_equal(got, e0[n]))
        if np.array_equal(ws[-1], e0[n]):      # a parameter that never moved comes back bit for bit
            assert got.tobytes() == e0[n].tobytes(), n
    assert moved > len(names) // 2
    print(f"   ema recurrence {name} {precision}: max err/bound {worst:.3f}, {moved}/{len(names)} entries moved")


# --------------------------------------------------------------------------------------------- 2. replay
def _replay_case(cfg, precision, N=1, warm=2, steps=5):
    from nvit_amd.train import GraphedTrainStep, train_step
    data = batches(cfg, B * N)
    me, oe, ee = with_ema(cfg, precision)
    mg, og, eg = with_ema(cfg, precision)      # attached before the capture
    kw = dict(accumulation_steps=N)
    for _ in range(warm):
        train_step(me, oe, *data[0], **kw)
    g = GraphedTrainStep(mg, og, *data[0], warmup=warm, **kw)
    assert g.ema is eg
    assert ee.updates == eg.updates == warm      # warm-up steps are updates, the capture pass is not
    assert_same_shadow(ee, eg, "after warm-up and capture")
    for i in range(steps):
        xb, yb = data[i % 3]
        le, lg = train_step(me, oe, xb, yb, **kw), g(xb, yb)
        assert torch.equal(le[0], lg[0]) and torch.equal(le[1], lg[1]), i
    assert ee.updates == eg.updates == warm + steps      # one update per optimizer step, whatever N is
    assert_same_shadow(ee, eg, "after the replays")
    assert_same_weights(me, mg, "after the replays")
    # eager and replayed steps alternating on one model
    for i, graphed in enumerate((False, True, False, True)):
        xb, yb = data[(i + 1) % 3]
        train_step(me, oe, xb, yb, **kw)
        (g if graphed else lambda X, y: train_step(mg, og, X, y, **kw))(xb, yb)
    assert ee.updates == eg.updates == warm + steps + 4
    assert_same_shadow(ee, eg, "after alternating steps")
    assert_same_weights(me, mg, "after alternating steps")
    assert same_bits(ee.state, eg.state)
    return eg


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["micro_k", "micro_k_fa"])
def test_replayed_steps_leave_the_bits_of_eager_steps(name, precision):
    eg = _replay_case(named_config(name, **SCHEDULE), precision)
    assert eg.renorm and not same_bits(eg.shadow["transformer.h.0.query.weight"],
                                       eg.model.transformer.h[0].query.weight)


def test_accumulation_is_one_update_per_optimizer_step():
    _replay_case(named_config("micro_k", **SCHEDULE), "bf16", N=2, steps=3)


# --------------------------------------------------------------------------------------------- 3. skip_nonfinite
@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_a_skipped_step_leaves_the_average_and_the_count(precision, graphed):
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = named_config("mini")
    (X0, y0), (X1, y1), (X2, y2) = batches(cfg)
    X1 = X1.clone()
    X1[B - 1, 1, 5, 7] = float("inf")      # one input pixel
    ma, oa, ea = with_ema(cfg, precision)
    if graphed:
        step = GraphedTrainStep(ma, oa, X0, y0, warmup=1, skip_nonfinite=True)      # its warm-up is the first step
    else:
        step = lambda X, y: train_step(ma, oa, X, y, skip_nonfinite=True)
        step(X0, y0)
    assert ea.updates == 1
    before, state = snapshot(ea), ea.state.clone()
    gnorm = step(X1, y1)[3]
    assert not torch.isfinite(gnorm).item() and oa.skipped_steps() == 1
    assert ea.updates == 1 and ea.state.tolist() == [1.0, 0.0, 0.0, 0.0] and state[1].item() > 0.0
    for n, t in ea.shadow.items():
        assert same_bits(t, before[n]), n
    step(X2, y2)
    assert ea.updates == 2 and ea.state[1].cpu().numpy().tobytes() == ema_ref.omd_at(1, 0.9998).tobytes()
    assert any(not same_bits(t, before[n]) for n, t in ea.shadow.items())
    # ... exactly as if the poisoned batch had never come: the unguarded twin that saw the two clean batches
    mb, ob, eb = with_ema(cfg, precision)
    train_step(mb, ob, X0, y0)
    train_step(mb, ob, X2, y2)
    assert_same_shadow(ea, eb, "after the recovery")
    assert_same_weights(ma, mb, "after the recovery")
    for t in ea.shadow.values():
        assert torch.isfinite(t).all()


# --------------------------------------------------------------------------------------------- 4. nViT module
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_nvit_module_is_the_renormalised_shadow(precision):
    from nvit_amd import ops
    from nvit_amd.optim import renorm_matrices
    from nvit_amd.train import train_step
    cfg = named_config("micro_k")
    data = batches(cfg)
    m, opt, ema = with_ema(cfg, precision)
    assert ema.renorm
    for k in range(3):
        train_step(m, opt, *data[k])
    before = snapshot(ema)
    mod = ema.module
    assert not mod.training and all(not p.requires_grad for p in mod.parameters())
    assert mod.config == m.config and mod.precision == precision
    assert mod.local_kohonen.locations is m.local_kohonen.locations      # integer buffers are shared
    ref = third_model(ema, cfg, precision)
    for (n, p), (_, q) in zip(mod.named_parameters(), ref.named_parameters()):
        assert same_bits(p, q), n
        assert p.data_ptr() != ema.shadow[n].data_ptr(), n      # separate tensors
    names = {id(p): n for n, p in mod.named_parameters()}
    mats = list(renorm_matrices(mod))
    assert len(mats) == 6 * cfg.n_layer
    worst = 0.0
    for w, dim in mats:
        src = before[names[id(w)]].cpu()
        r = oc.renorm_eval(src, dim)
        _, bnd = oc.renorm_bounds(src, dim)
        nerr = (w.detach().cpu().double().norm(dim=dim) - 1).abs()
        nb = oc.unit_norm_bound(r, bnd, dim)
        assert (nerr <= nb).all(), (names[id(w)], dim, (nerr / nb).max().item())
        worst = max(worst, (nerr / nb).max().item())
    # sync() leaves the shadow alone, and is one copy launch plus the stand-alone renorm
    ops.prof_enable(True)
    try:
        ops.prof_collect()
        ema.sync()
        prof = ops.prof_collect()
    finally:
        ops.prof_enable(False)
    assert {k: v["launches"] for k, v in prof.items() if v["launches"]} == {"optim": 1, "renorm": 1}
    for n, t in ema.shadow.items():
        assert same_bits(t, before[n]), n
    for (n, p), (_, q) in zip(mod.named_parameters(), ref.named_parameters()):
        assert same_bits(p, q), n
    # the next update makes the module stale, and the property refreshes it
    train_step(m, opt, *data[0])
    assert ema.module is mod
    ref2 = third_model(ema, cfg, precision)
    assert any(not same_bits(p, q) for p, q in zip(ref.parameters(), ref2.parameters()))
    for (n, p), (_, q) in zip(mod.named_parameters(), ref2.named_parameters()):
        assert same_bits(p, q), n
    print(f"   ema module {precision}: unit norm err/bound {worst:.3f}")


# --------------------------------------------------------------------------------------------- 5. plain ViT
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_plain_vit_module_shares_the_shadow(precision):
    from nvit_amd import ops
    from nvit_amd.train import train_step
    cfg = named_config("micro_vit")
    data = batches(cfg)
    m, opt, ema = with_ema(cfg, precision)
    assert not ema.renorm
    for k in range(2):
        train_step(m, opt, *data[k])
    ops.prof_enable(True)
    try:
        ops.prof_collect()
        ema.sync()
        mod = ema.module
        prof = ops.prof_collect()
    finally:
        ops.prof_enable(False)
    assert all(v["launches"] == 0 for v in prof.values()), prof
    storage = {p.untyped_storage().data_ptr() for p in mod.parameters()}
    assert len(storage) == 1      # the one flat buffer
    for n, p in mod.named_parameters():
        s = ema.shadow[n]
        assert p.data_ptr() == s.data_ptr() and p.shape == s.shape and p.data_ptr() % 16 == 0, n
        assert same_bits(p, s) and not p.requires_grad, n
    train_step(m, opt, *data[2])      # the module sees the update without any copy
    for n, p in ema.module.named_parameters():
        assert p.data_ptr() == ema.shadow[n].data_ptr() and same_bits(p, ema.shadow[n]), n
    assert ema.updates == 3


# --------------------------------------------------------------------------------------------- 6. evaluation
@pytest.mark.parametrize("name", ["micro_k", "micro_vit"])
def test_evaluation_through_the_module(name):
    from nvit_amd.evaluate import GraphedEval, estimate_loss, predict, validate
    from nvit_amd.train import train_step
    cfg = named_config(name)
    data = batches(cfg)
    m, opt, ema = with_ema(cfg, "bf16")
    for k in range(2):
        train_step(m, opt, *data[k])
    ref = third_model(ema, cfg, "bf16")
    X = data[2][0]
    assert validate(ema.module, data) == validate(ref, data)
    assert torch.equal(predict(ema.module, X), predict(ref, X))
    assert estimate_loss(ema.module, data, 2) == estimate_loss(ref, data, 2)
    assert not ema.module.training and m.training
    g = GraphedEval(ema.module, *data[0])
    stale = g.validate(data)
    for k in range(2):
        train_step(m, opt, *data[k])
    ema.sync()
    fresh = validate(ema.module, data)
    assert g.validate(data) == fresh and fresh != stale
    assert torch.equal(g.predict(X), predict(ema.module, X))
    assert validate(third_model(ema, cfg, "bf16"), data) == fresh


# --------------------------------------------------------------------------------------------- 7. attach / detach
def test_without_an_attached_ema_nothing_changes(tmp_path):
    """Against a fresh process that never imported nvit_amd.ema: a run in this process with no EMA attached, and one
    where an EMA was constructed, attached and detached again before the first step."""
    from nvit_amd import ModelEma
    out = tmp_path / "plain.npz"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ema_worker.py"), str(out)], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:]
    want = dict(np.load(out))
    assert want["steps"] == ema_worker.K + 3 and len(want) > 50

    def attach_and_detach(m, opt):
        ema = ModelEma(m)
        opt.attach_ema(ema)
        opt.attach_ema(None)

    for what, hook in (("never attached", None), ("attached and detached", attach_and_detach)):
        got = ema_worker.run(hook)
        assert set(got) == set(want), what
        for k in want:
            assert got[k].tobytes() == want[k].tobytes(), (what, k)


def test_graphed_step_refuses_another_ema_than_the_captured_one():
    from nvit_amd import ModelEma
    from nvit_amd.train import GraphedTrainStep
    cfg = named_config("micro_k")
    X, y = batches(cfg)[0]
    m, opt, ema = with_ema(cfg, "bf16")
    g = GraphedTrainStep(m, opt, X, y, warmup=1)
    g(X, y)
    weights, n = [p.detach().clone() for p in m.parameters()], ema.updates
    for other in (None, ModelEma(m)):
        opt.attach_ema(other)
        with pytest.raises(ValueError, match="captured with another ModelEma"):
            g(X, y)
    opt.attach_ema(ema)
    assert ema.updates == n and all(same_bits(p, w) for p, w in zip(m.parameters(), weights))
    g(X, y)
    assert ema.updates == n + 1
    # ... and the other way round: captured without, called with one attached
    m2 = build(cfg, "bf16")
    opt2 = optimizer(m2)
    g2 = GraphedTrainStep(m2, opt2, X, y, warmup=1)
    assert g2.ema is None
    opt2.attach_ema(ModelEma(m2))
    with pytest.raises(ValueError, match="captured with another ModelEma"):
        g2(X, y)
    opt2.attach_ema(None)
    g2(X, y)


# --------------------------------------------------------------------------------------------- 8. checkpoint
@pytest.mark.parametrize("name", ["micro_k", "micro_vit"])
def test_checkpoint_round_trip_on_the_device(name, tmp_path):
    from nvit_amd import ModelEma
    from nvit_amd.checkpoint import load_checkpoint, save_checkpoint
    from nvit_amd.train import train_step
    cfg = named_config(name)
    data = batches(cfg)
    m, opt, ema = with_ema(cfg, "bf16", decay=0.99)
    for k in range(2):
        train_step(m, opt, *data[k])
    path = save_checkpoint(tmp_path / "ck.pt", m, opt, 2, {"val/loss": 0.0}, ema=ema)
    m2, opt2, ck = load_checkpoint(path, device="cuda:0", optimizer_factory=optimizer, restore_rng=False)
    m2.set_precision("bf16").train()
    m2.step, m2.total_steps = m.step, m.total_steps
    sd = ck["model_ema"]
    assert sd["updates"] == 2 and sd["decay"] == 0.99 and sd["warmup"] is True
    assert all(t.device.type == "cpu" and t.dtype == torch.float32 for t in sd["shadow"].values())
    ema2 = ModelEma(m2)      # default decay: the loaded state overrides it
    ema2.load_state_dict(sd)
    opt2.attach_ema(ema2)
    assert ema2.updates == 2 and ema2.decay == 0.99
    assert_same_shadow(ema, ema2, "after loading")
    train_step(m, opt, *data[2])
    train_step(m2, opt2, *data[2])
    assert ema.updates == ema2.updates == 3 and same_bits(ema.state, ema2.state)
    assert_same_shadow(ema, ema2, "one step after loading")
    assert_same_weights(m, m2, "one step after loading")
    if ema.renorm:
        for (n, p), (_, q) in zip(ema.module.named_parameters(), ema2.module.named_parameters()):
            assert same_bits(p, q), n
    with pytest.raises(RuntimeError):
        ema2.load_state_dict({**sd, "shadow": {k: v for k, v in list(sd["shadow"].items())[1:]}})
