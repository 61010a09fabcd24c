"""CPU: the public face of the device learning-rate schedule (nvit_amd.LRSchedule, layer_decay_groups,
ViT.configure_optimizers(layer_decay=), the checkpoint key) and the host restatement `lr_at` against the twin
lr_schedule_ref.py, bit for bit.  No device work."""
import math

import pytest
import torch

import lr_schedule_ref as lr_ref

SHIPPED = dict(lr=1e-3, min_lr=1e-5, W=5, D=20)


def _bits(x):
    return lr_ref.f64_bits(x)


@pytest.mark.parametrize("W", [5, 0])
def test_lr_at_is_the_reference_get_lr_bit_for_bit(W):
    from nvit_amd import LRSchedule
    lr, min_lr, D = SHIPPED["lr"], SHIPPED["min_lr"], SHIPPED["D"]
    sched = LRSchedule.from_reference(lr, min_lr, W, D)
    assert (sched.kind, sched.warmup_init) == ("cosine", 0.0)
    for s in range(D + 4):
        want = lr_ref.get_lr(s, lr, min_lr, W, D)
        assert _bits(sched.lr_at(s)) == _bits(want), (s, sched.lr_at(s), want)
        assert _bits(lr_ref.closed_form("cosine", s, lr, min_lr, W, D)) == _bits(want)
    same = LRSchedule("cosine", lr, min_lr, W, D)
    assert all(_bits(same.lr_at(s)) == _bits(sched.lr_at(s)) for s in range(D + 4))


def test_edge_values_are_exact():
    from nvit_amd import LRSchedule
    lr, min_lr, W, D = SHIPPED["lr"], SHIPPED["min_lr"], SHIPPED["W"], SHIPPED["D"]
    for kind in ("cosine", "linear"):
        sched = LRSchedule(kind, lr, min_lr, W, D)
        assert sched.lr_at(0) == 0.0
        assert sched.lr_at(W) == lr            # r = 0: cos(0) = 1, coefficient exactly 1
        if kind == "cosine":
            assert sched.lr_at(D) == min_lr    # r = 1: cos(pi) == -1.0, coefficient exactly 0
        else:                                  # the stated form lr + (min_lr - lr) * 1.0 rounds twice: within an ulp of lr
            assert sched.lr_at(D) == lr + (min_lr - lr) * 1.0 and abs(sched.lr_at(D) - min_lr) <= 2.0 ** -52 * lr
        assert sched.lr_at(D + 1) == min_lr and sched.lr_at(D + 1000) == min_lr
        assert min_lr < sched.lr_at((W + D) // 2) < lr
    assert math.cos(math.pi) == -1.0
    # the reference's warm-up is lr * s / W exactly, not (lr / W) * s
    sched = LRSchedule("cosine", lr, min_lr, 7, D)
    assert all(_bits(sched.lr_at(s)) == _bits(lr * s / 7) for s in range(7))


def test_linear_and_constant_kinds_and_warmup_init():
    from nvit_amd import LRSchedule
    lr, min_lr, W, D = 3e-4, 2e-6, 4, 13
    lin = LRSchedule("linear", lr, min_lr, W, D)
    for s in range(W, D + 1):
        assert _bits(lin.lr_at(s)) == _bits(lr + (min_lr - lr) * ((s - W) / (D - W)))
    const = LRSchedule("constant", lr, warmup_iters=W)
    assert [const.lr_at(s) for s in (W, W + 1, 10 ** 9)] == [lr] * 3
    assert const.lr_at(1) == lr * 1 / W
    assert LRSchedule("constant", lr, min_lr, W, 2).lr_at(50) == lr     # D is ignored, even D <= W
    assert LRSchedule("constant", lr).lr_at(0) == lr
    for kind in ("cosine", "linear", "constant"):
        sched = LRSchedule(kind, lr, min_lr, W, D, warmup_init=1e-6)
        assert sched.lr_at(0) == 1e-6
        for s in range(D + 4):
            want = lr_ref.closed_form(kind, s, lr, min_lr, W, D, 1e-6)
            assert _bits(sched.lr_at(s)) == _bits(want), (kind, s)
        for s in range(W):
            assert _bits(sched.lr_at(s)) == _bits(1e-6 + (lr - 1e-6) * s / W)
        assert all(sched.lr_at(s) < sched.lr_at(s + 1) for s in range(W))


def test_constructor_validation():
    from nvit_amd import LRSchedule
    with pytest.raises(ValueError):
        LRSchedule("exponential", 1e-3, 0.0, 0, 10)
    with pytest.raises(ValueError):
        LRSchedule("cosine", 1e-3, 0.0, -1, 10)            # W >= 0
    for kind in ("cosine", "linear"):
        for W, D in ((5, 5), (5, 4), (0, 0)):
            with pytest.raises(ValueError):
                LRSchedule(kind, 1e-3, 0.0, W, D)          # D > W
        with pytest.raises(ValueError):
            LRSchedule(kind, 1e-3, 0.0, 2)                 # no D at all
    for bad in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            LRSchedule("cosine", bad, 0.0, 0, 10)
        with pytest.raises(ValueError):
            LRSchedule("cosine", 1e-3, bad, 0, 10)
        with pytest.raises(ValueError):
            LRSchedule("cosine", 1e-3, 0.0, 0, 10, warmup_init=bad)
    with pytest.raises(TypeError):
        LRSchedule("cosine", "1e-3", 0.0, 0, 10)
    with pytest.raises(TypeError):
        LRSchedule("cosine", 1e-3, 0.0, 1.5, 10)
    with pytest.raises(ValueError):
        LRSchedule.from_reference(1e-3, 1e-5, 20, 20)
    sched = LRSchedule("cosine", 1e-3, 1e-5, 0, 2 ** 31 + 10)
    assert sched.decay_iters == 2 ** 31 + 10 and sched.step == 0
    with pytest.raises(RuntimeError):
        sched.apply()                                      # no device yet
    with pytest.raises(RuntimeError):
        sched.last_lr
    with pytest.raises(RuntimeError):
        sched.to("cpu")


def test_state_dict_round_trip(tmp_path):
    from nvit_amd import LRSchedule
    sched = LRSchedule("linear", 2e-3, 1e-6, 3, 2 ** 33, warmup_init=1e-7)
    state = sched.state_dict()
    assert state == {"kind": "linear", "lr": 2e-3, "min_lr": 1e-6, "warmup_iters": 3, "decay_iters": 2 ** 33,
                     "warmup_init": 1e-7, "step": 0}
    state["step"] = 2 ** 31 + 3
    sched.load_state_dict(state)
    assert sched.step == 2 ** 31 + 3 and sched.state_dict() == state
    torch.save(sched.state_dict(), tmp_path / "s.pt")
    other = LRSchedule("constant", 1.0)
    other.load_state_dict(torch.load(tmp_path / "s.pt", weights_only=True))
    assert other.state_dict() == state and other.kind == "linear"
    assert _bits(other.lr_at(10 ** 6)) == _bits(sched.lr_at(10 ** 6))
    with pytest.raises(ValueError):
        other.load_state_dict(dict(state, step=-1))
    with pytest.raises(ValueError):
        other.load_state_dict(dict(state, decay_iters=3))
    assert other.state_dict() == state                     # a refused load leaves it as it was


def test_checkpoint_key_set():
    from nvit_amd import LRSchedule, ViT, named_config
    from nvit_amd.checkpoint import build_checkpoint
    m = ViT(named_config("micro"))
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    base = build_checkpoint(m, opt, 3, {"loss": 1.0})
    assert "lr_schedule" not in base
    sched = LRSchedule.from_reference(1e-3, 1e-5, 5, 20)
    sched.load_state_dict(dict(sched.state_dict(), step=42))
    ck = build_checkpoint(m, opt, 3, {"loss": 1.0}, lr_schedule=sched)
    assert set(ck) == set(base) | {"lr_schedule"} and ck["lr_schedule"] == sched.state_dict()
    assert ck["lr_schedule"]["step"] == 42


def _ids(groups):
    return [id(p) for g in groups for p in g["params"]]


@pytest.mark.parametrize("name", ["mini", "mini_vit", "micro_k"])
def test_layer_decay_groups(name):
    from nvit_amd import ViT, layer_decay_groups, named_config
    cfg = named_config(name)
    m = ViT(cfg)
    L = cfg.n_layer
    today = m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cpu").param_groups
    groups = layer_decay_groups(m, 0.1, 1e-3, 0.75)
    ids = _ids(groups)
    assert len(ids) == len(set(ids)) and set(ids) == set(_ids(today))         # every parameter, once
    names = {id(p): n for n, p in m.named_parameters()}
    decayed = {id(p) for p in today[0]["params"]}
    seen_depths = set()
    for g in groups:
        d = g["depth"]
        seen_depths.add(d)
        assert g["lr_scale"] == 0.75 ** (L + 2 - d) and g["lr"] == 1e-3 * g["lr_scale"]
        for p in g["params"]:
            n = names[id(p)]
            if n.startswith(("local_patch_embed.", "global_patch_embed.")) or n.endswith("_pos_embed"):
                want = 0
            elif n.startswith("cross_attention."):
                want = 1
            elif n.startswith("transformer.h."):
                want = int(n.split(".")[2]) + 2
            else:
                want = L + 2
            assert d == want, (n, d, want)
            assert g["weight_decay"] == (0.1 if id(p) in decayed else 0.0), n
    assert seen_depths == set(range(L + 3))
    top = [g for g in groups if g["depth"] == L + 2]
    assert all(g["lr_scale"] == 1.0 and g["lr"] == 1e-3 for g in top)
    head = {names[id(p)] for g in top for p in g["params"]}
    assert "mlp_head.1.weight" in head and (not cfg.use_nvit or "sz" in head)
    if cfg.use_kohonen:
        assert any(n.startswith("reconstruction_head.") for n in head)
    for bad in (0.0, -0.5, float("nan")):
        with pytest.raises(ValueError):
            layer_decay_groups(m, 0.1, 1e-3, bad)


def test_configure_optimizers_layer_decay_keyword():
    from nvit_amd import ViT, layer_decay_groups, named_config
    m = ViT(named_config("mini"))
    today = m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cpu")
    none = m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cpu", layer_decay=None)
    assert len(none.param_groups) == len(today.param_groups) == 3
    for a, b in zip(none.param_groups, today.param_groups):
        assert a.keys() == b.keys() and "lr_scale" not in a
        assert [id(p) for p in a["params"]] == [id(p) for p in b["params"]]
        assert (a["lr"], a["weight_decay"], a["betas"]) == (b["lr"], b["weight_decay"], b["betas"])
    opt = m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cpu", layer_decay=0.75)
    want = layer_decay_groups(m, 0.1, 1e-3, 0.75)
    assert len(opt.param_groups) == len(want)
    for a, b in zip(opt.param_groups, want):
        assert [id(p) for p in a["params"]] == [id(p) for p in b["params"]]
        assert (a["lr"], a["lr_scale"], a["weight_decay"]) == (b["lr"], b["lr_scale"], b["weight_decay"])
        assert a["betas"] == (0.9, 0.95)
    with pytest.raises(TypeError):
        m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cpu", 0.75)            # keyword only


def test_attach_schedule_on_the_optimizer():
    from nvit_amd import FusedAdamW, LRSchedule
    p = torch.nn.Parameter(torch.zeros(4))
    opt = FusedAdamW([p], lr=1e-3)
    assert opt.schedule is None
    sched = LRSchedule("constant", 1e-3)
    opt.attach_schedule(sched)
    assert opt.schedule is sched and opt.param_groups[0]["lr"] == 1e-3
    opt.attach_schedule(None)
    assert opt.schedule is None
    with pytest.raises(TypeError):
        opt.attach_schedule(1e-3)
    with pytest.raises(RuntimeError):
        opt.current_lr()


def test_kind_codes_come_from_the_header():
    from nvit_amd import _lib, schedule
    assert schedule.KINDS == {"cosine": _lib.const("LR_COSINE"), "linear": _lib.const("LR_LINEAR"),
                              "constant": _lib.const("LR_CONSTANT")}
    assert len(set(schedule.KINDS.values())) == 3 and schedule.THREADS == _lib.const("LR_SCHEDULE_THREADS")
