"""GPU tests, model level, of the device learning-rate schedule (FusedAdamW.attach_schedule): W = 2, D = 5, so six steps
cross the warm-up, the cosine segment and the floor.  A run with the schedule attached must be, bit for bit, the run whose
host loop sets group["lr"] to the fp32 rates the schedule kernel produces (read from a stand-alone schedule) - eagerly,
replayed, with gradient accumulation, with a skipped step, across a resume, and with layer-wise lr decay - and nothing may
change when nothing is attached.  Run on the MI355X box: pytest -m gpu."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lr_schedule_ref as lr_ref
from nvit_amd.config import named_config
from nvit_amd.weights import formula_state_dict, synthetic_batch

LR, MIN_LR, W, D = 1e-3, 1e-5, 2, 5
CONFIGS = [("mini", "fp32"), ("mini", "bf16"), ("micro_k", "bf16"), ("mini_vit", "fp32")]


def build(cfg, precision):
    from nvit_amd.model import ViT
    from nvit_amd.train import normalize_matrices
    m = ViT(cfg)
    res = m.load_state_dict(formula_state_dict(cfg), strict=False)
    assert not res.unexpected_keys and all(k.endswith((".locations", ".offsets")) for k in res.missing_keys)
    m = m.to("cuda:0").set_precision(precision).train()
    normalize_matrices(m)
    return m


def optimizer(m, **kw):
    return m.configure_optimizers(0.1, LR, (0.9, 0.95), "cuda", **kw)


def schedule(kind="cosine", w=W):
    from nvit_amd import LRSchedule
    return LRSchedule(kind, LR, MIN_LR, w, D).to("cuda:0")


def batches(cfg, rows=4):
    return [tuple(t.cuda() for t in synthetic_batch(cfg, rows, seed=s)) for s in (1234, 77)]


_RATES = {}


def device_rates(n=6):
    """The fp32 rate the schedule kernel produces for steps 0..n-1, from a stand-alone schedule; computed once."""
    if n not in _RATES:
        sched, out = schedule(), []
        for _ in range(n):
            sched.apply()
            out.append(float(sched.last_lr.item()))
        assert sched.step == n
        for s, v in enumerate(out):     # the twin, to the op-level bound (scale 1)
            L = lr_ref.closed_form("cosine", s, LR, MIN_LR, W, D)
            assert abs(v - L) <= lr_ref.row_bound(L, 1.0, LR), (s, v, L)
        assert out[0] == 0.0 and out[2] == np.float32(LR) and out[5] == np.float32(MIN_LR) and out[2] > out[3] > out[4] > out[5]
        _RATES[n] = tuple(out)
    return _RATES[n]


def set_lr(opt, lr):
    for g in opt.param_groups:
        g["lr"] = float(lr)


def same_run(ma, mb, oa, ob, what=""):
    n = 0
    for (name, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.isfinite(pa).all(), (what, name)
        assert torch.equal(pa, pb), (what, name)
        if pa in oa.state:
            n += 1
            for key in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(oa.state[pa][key], ob.state[pb][key]), (what, name, key)
    assert n > 10
    if ma.config.use_kohonen:
        assert torch.equal(ma.local_kohonen.nodes, mb.local_kohonen.nodes), what
        assert torch.equal(ma.global_kohonen.nodes, mb.global_kohonen.nodes), what


def differ(ma, mb):
    return any(not torch.equal(pa, pb) for pa, pb in zip(ma.parameters(), mb.parameters()))


@pytest.mark.parametrize("name,precision", CONFIGS)
def test_attached_schedule_is_the_hand_loop(name, precision):
    from nvit_amd.train import train_step
    cfg = named_config(name)
    data = batches(cfg)
    rates = device_rates()
    ma, mb, mc = build(cfg, precision), build(cfg, precision), build(cfg, precision)
    oa, ob, oc = optimizer(ma), optimizer(mb), optimizer(mc)
    sched = schedule()
    oa.attach_schedule(sched)
    assert oa.schedule is sched
    for i in range(6):
        X, y = data[i % 2]
        la = train_step(ma, oa, X, y)
        set_lr(ob, rates[i])
        lb = train_step(mb, ob, X, y)
        train_step(mc, oc, X, y)
        assert torch.equal(la[0], lb[0]) and torch.equal(la[1], lb[1]) and torch.equal(la[3], lb[3]), i
        assert sched.last_lr.item() == np.float32(rates[i])
    same_run(ma, mb, oa, ob, name)
    assert differ(ma, mc)                                    # the schedule does change the run
    assert sched.step == 6 and oa.current_lr() == rates[5]
    assert all(g["lr"] == LR for g in oa.param_groups)       # the groups keep the peak rate
    # an off-by-one in s is another run: the hand loop one step late
    md = build(cfg, precision)
    od = optimizer(md)
    for i in range(6):
        set_lr(od, rates[max(i - 1, 0)])
        train_step(md, od, *data[i % 2])
    assert differ(ma, md)


@pytest.mark.parametrize("name,precision", CONFIGS[:3])
def test_replay_is_eager(name, precision):
    """warm-up 2 + 4 replays on one model, and warm-up 1 + replays and eager steps alternating on another, against six eager
    steps; set_lr and a call with another schedule attached are refused."""
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = named_config(name)
    (X, y), (X2, y2) = batches(cfg)
    order = [(X, y), (X, y), (X2, y2), (X, y), (X2, y2), (X, y)]
    me, mg, mh = build(cfg, precision), build(cfg, precision), build(cfg, precision)
    oe, og, oh = optimizer(me), optimizer(mg), optimizer(mh)
    se, sg, sh = schedule(), schedule(), schedule()
    for o, s in ((oe, se), (og, sg), (oh, sh)):
        o.attach_schedule(s)
    eager = [train_step(me, oe, xb, yb) for xb, yb in order]
    g = GraphedTrainStep(mg, og, X, y, warmup=2)
    assert sg.step == 2                                      # the capture pass is no schedule step
    for i in range(2, 6):
        out = g(*order[i])
        assert torch.equal(out[0], eager[i][0]) and torch.equal(out[1], eager[i][1]) and torch.equal(out[3], eager[i][3]), i
        assert torch.equal(sg.last_lr, torch.tensor([device_rates()[i]], device="cuda:0"))
    same_run(me, mg, oe, og, "replayed")
    assert sg.step == se.step == 6
    h = GraphedTrainStep(mh, oh, X, y, warmup=1)
    for i in range(1, 6):
        out = h(*order[i]) if i % 2 else train_step(mh, oh, *order[i])
        assert torch.equal(out[0], eager[i][0]) and torch.equal(out[1], eager[i][1]), i
    same_run(me, mh, oe, oh, "alternating")
    assert sh.step == 6
    with pytest.raises(ValueError):
        g.set_lr(5e-4)
    assert all(grp["lr"] == LR for grp in og.param_groups)
    og.attach_schedule(schedule())
    with pytest.raises(ValueError):
        g(X, y)
    og.attach_schedule(None)
    with pytest.raises(ValueError):
        g(X, y)
    og.attach_schedule(sg)
    g(X, y)
    assert sg.step == 7


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
def test_one_optimizer_step_is_one_schedule_step_under_accumulation(graphed):
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = named_config("mini")
    data = batches(cfg, rows=8)
    rates = device_rates()
    ma, mb = build(cfg, "bf16"), build(cfg, "bf16")
    oa, ob = optimizer(ma), optimizer(mb)
    sched = schedule()
    oa.attach_schedule(sched)
    if graphed:
        g = GraphedTrainStep(ma, oa, *data[0], warmup=1, accumulation_steps=2)
    for i in range(4):
        X, y = data[0] if i == 0 else data[i % 2]
        if graphed and i > 0:
            g(X, y)
        elif not graphed:
            train_step(ma, oa, X, y, accumulation_steps=2)
        set_lr(ob, rates[i])
        train_step(mb, ob, X, y, accumulation_steps=2)
    assert sched.step == 4
    same_run(ma, mb, oa, ob)


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
def test_a_skipped_step_is_a_schedule_step(graphed):
    """five batches, the third poisoned: the schedule counter reads 5, one step was skipped, and the weights are those of
    the hand loop that leaves that step's update out but still advances i"""
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = named_config("mini")       # no Kohonen head: no index is derived from a NaN distance
    data = batches(cfg)
    rates = device_rates()
    bad = data[0][0].clone()
    bad[3, 1, 5, 7] = float("nan")
    ma, mb = build(cfg, "bf16"), build(cfg, "bf16")
    oa, ob = optimizer(ma), optimizer(mb)
    sched = schedule()
    oa.attach_schedule(sched)
    if graphed:
        g = GraphedTrainStep(ma, oa, *data[0], warmup=1, skip_nonfinite=True)
    for i in range(5):
        X, y = (bad, data[0][1]) if i == 2 else data[0] if i == 0 else data[i % 2]
        if graphed and i > 0:
            g(X, y)
        elif not graphed:
            train_step(ma, oa, X, y, skip_nonfinite=True)
        if i != 2:
            set_lr(ob, rates[i])
            train_step(mb, ob, X, y)
    assert sched.step == 5 and oa.skipped_steps() == 1
    same_run(ma, mb, oa, ob)
    steps = {int(float(st["step"])) for st in oa.state_dict()["state"].values()}
    assert steps == {4}


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
def test_resume_from_state_dicts(graphed):
    """three steps, the state_dicts of model, optimizer and schedule into fresh objects, three more = six uninterrupted"""
    from nvit_amd import LRSchedule
    from nvit_amd.train import GraphedTrainStep, train_step
    cfg = named_config("mini")
    X, y = batches(cfg)[0]
    ma = build(cfg, "bf16")
    oa = optimizer(ma)
    sa = schedule()
    oa.attach_schedule(sa)
    for _ in range(6):
        want = train_step(ma, oa, X, y)

    def three(m, o):
        if graphed:
            g = GraphedTrainStep(m, o, X, y, warmup=1)
            g(X, y)
            return g(X, y)
        train_step(m, o, X, y)
        train_step(m, o, X, y)
        return train_step(m, o, X, y)

    mb = build(cfg, "bf16")
    ob = optimizer(mb)
    sb = schedule()
    ob.attach_schedule(sb)
    three(mb, ob)
    saved = copy.deepcopy({"model": mb.state_dict(), "optimizer": ob.state_dict(), "lr_schedule": sb.state_dict()})
    assert saved["lr_schedule"]["step"] == 3
    mc = build(cfg, "bf16")
    mc.load_state_dict(saved["model"])
    oc = optimizer(mc)
    oc.load_state_dict(saved["optimizer"])
    sc = LRSchedule("constant", 1.0)
    sc.load_state_dict(saved["lr_schedule"])
    sc.to("cuda:0")
    oc.attach_schedule(sc)
    got = three(mc, oc)
    assert sc.step == 6
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[3], want[3])
    same_run(ma, mc, oa, oc)


def test_layer_decay_rows_and_hand_loop():
    from nvit_amd import _lib
    from nvit_amd.train import train_step
    cfg = named_config("mini")
    data = batches(cfg)
    ma, mb = build(cfg, "fp32"), build(cfg, "fp32")
    oa, ob = optimizer(ma, layer_decay=0.75), optimizer(mb, layer_decay=0.75)
    L = cfg.n_layer
    assert sorted({g["lr_scale"] for g in oa.param_groups}) == sorted(0.75 ** k for k in range(L + 3))
    sched = schedule(w=0)                                    # both steps inside the cosine segment, at rates above 0
    oa.attach_schedule(sched)
    cols = _lib.const("OPT_TABLE_COLS")
    for s in range(2):
        X, y = data[s]
        train_step(ma, oa, X, y)
        c = oa._cache
        assert c["table"].shape == (c["n"], cols) and len(c["groups"]) == c["n"] > len(oa.param_groups)
        rows = (c["table"][:, -1].cpu() & 0xFFFFFFFF).numpy().astype(np.uint32).view(np.float32)
        Ls = sched.lr_at(s)
        per_group = {}
        for i, gi in enumerate(c["groups"]):
            grp = oa.param_groups[gi]
            scale = np.float32(0.75 ** (L + 2 - grp["depth"]))
            assert np.float32(grp["lr_scale"]) == scale
            assert abs(float(rows[i]) - Ls * float(scale)) <= lr_ref.row_bound(Ls, scale, LR), (s, i, rows[i])
            assert per_group.setdefault(gi, rows[i]) == rows[i]
        wd = (c["table"][:, -1].cpu() >> 32).numpy().astype(np.uint32).view(np.float32)
        assert all(wd[i] == np.float32(oa.param_groups[gi]["weight_decay"]) for i, gi in enumerate(c["groups"]))
        for gi, grp in enumerate(ob.param_groups):
            grp["lr"] = float(per_group[gi])
        train_step(mb, ob, X, y)
    assert len(set(per_group.values())) == L + 3
    same_run(ma, mb, oa, ob)


@pytest.mark.parametrize("name,precision", [("mini", "bf16"), ("micro_k", "bf16")])
def test_nothing_attached_and_a_constant_schedule_are_the_same_bits(name, precision):
    """the attached path changes no arithmetic: kind constant, W = 0, at the groups' lr; and a detached schedule leaves the
    groups' lr in force again"""
    from nvit_amd import LRSchedule
    from nvit_amd.train import train_step
    cfg = named_config(name)
    data = batches(cfg)
    ma, mb = build(cfg, precision), build(cfg, precision)
    oa, ob = optimizer(ma), optimizer(mb)
    sched = LRSchedule("constant", LR).to("cuda:0")
    ob.attach_schedule(sched)
    for i in range(3):
        la = train_step(ma, oa, *data[i % 2])
        lb = train_step(mb, ob, *data[i % 2])
        assert torch.equal(la[0], lb[0]) and torch.equal(la[1], lb[1]) and torch.equal(la[3], lb[3])
    same_run(ma, mb, oa, ob)
    assert sched.step == 3 and ob.current_lr() == float(np.float32(LR))
    ob.attach_schedule(None)
    la = train_step(ma, oa, *data[1])
    lb = train_step(mb, ob, *data[1])
    assert torch.equal(la[0], lb[0]) and sched.step == 3
    same_run(ma, mb, oa, ob)
