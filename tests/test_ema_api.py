"""CPU: the surface of the weight EMA (nvit_amd.ModelEma): export, C entry points, argument refusals, the optimizer
hook, the unchanged train-step signatures, the checkpoint key, and the decay formula of tests/ema_ref.py."""
import ctypes
import inspect
import os
import re
import sys

import pytest
import torch

import ema_ref
from nvit_amd.config import named_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_KEYS = {"model", "optimizer", "model_args", "iter_num", "metrics", "config", "rng_state_pytorch",
            "rng_state_numpy", "timestamp"}
ENTRY_POINTS = ("nvit_ema_tick", "nvit_ema_update")


def _lib_path():
    from nvit_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return _lib.LIB_PATH


def test_model_ema_is_exported_lazily():
    import nvit_amd
    from nvit_amd.ema import ModelEma
    assert nvit_amd.ModelEma is ModelEma
    assert list(inspect.signature(ModelEma.__init__).parameters)[1:] == ["model", "decay", "warmup", "renorm"]
    d = {p.name: p.default for p in inspect.signature(ModelEma.__init__).parameters.values()}
    assert (d["decay"], d["warmup"], d["renorm"]) == (0.9998, True, None)
    for name in ("update", "sync", "state_dict", "load_state_dict"):
        assert callable(getattr(ModelEma, name)), name
    assert isinstance(ModelEma.module, property) and isinstance(ModelEma.updates, property)


def test_entry_points_are_declared_bound_and_exported():
    from nvit_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "nvit_hip.h")).read()
    lib = ctypes.CDLL(_lib_path())
    loaded = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name) and hasattr(loaded, name), name
    assert _lib.SIGNATURES["nvit_ema_tick"][1] is ctypes.c_double   # the decay crosses the boundary as a double
    mk = open(os.path.join(ROOT, "nvit_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, re.M).group(1).split()
    src = "ema.hip" if os.path.exists(os.path.join(ROOT, "nvit_amd", "csrc", "ema.hip")) else "optim.hip"
    assert src in srcs and "nvit_ema_update" in open(os.path.join(ROOT, "nvit_amd", "csrc", src)).read()
    for name in ("EMA_TABLE_COLS", "EMA_CHUNK", "EMA_MAX_GRID", "EMA_FLAG_COPY", "EMA_FLAG_SCALAR"):
        assert getattr(ops, name) == _lib.const(name), name
    assert ops.EMA_CHUNK % 1024 == 0 and ops.EMA_FLAG_COPY != ops.EMA_FLAG_SCALAR
    for name in ("ema_table", "ema_tick", "ema_update"):
        assert callable(getattr(ops, name)), name
    assert _lib.const("KID_COUNT") == 15   # no new profiling family: the launches count under "optim"


@pytest.fixture(scope="module")
def cpu_model():
    from nvit_amd.model import ViT
    return ViT(named_config("micro"))


@pytest.mark.parametrize("decay", [-0.1, 1.0, 1.5, float("nan")])
def test_decay_outside_the_half_open_unit_interval_is_refused(cpu_model, decay):
    from nvit_amd import ModelEma
    with pytest.raises(ValueError):
        ModelEma(cpu_model, decay=decay)


def test_cpu_resident_model_is_refused_with_the_models_own_error(cpu_model):
    from nvit_amd import ModelEma
    before = {k: v.clone() for k, v in cpu_model.state_dict().items()}
    training, rng = cpu_model.training, torch.get_rng_state()
    with pytest.raises(RuntimeError) as e:
        ModelEma(cpu_model)
    with pytest.raises(RuntimeError) as own:
        cpu_model._prepare(torch.device("cpu"))
    assert str(e.value) == str(own.value)
    assert cpu_model.training == training and torch.equal(torch.get_rng_state(), rng)
    after = cpu_model.state_dict()
    assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert all(p.device.type == "cpu" and p.requires_grad for p in cpu_model.parameters())


class _StubEma:
    """What the optimizer and the checkpoint ask of a ModelEma; its device side needs the GPU."""

    def __init__(self):
        self.calls, self.dirty = [], 0

    def update(self, skip_state=None):
        self.calls.append(skip_state)

    def mark_dirty(self):
        self.dirty += 1

    def state_dict(self):
        return {"shadow": {"w": torch.arange(6, dtype=torch.float32).reshape(2, 3)}, "updates": 3, "decay": 0.99,
                "warmup": True}


def test_attach_and_detach(cpu_model):
    from nvit_amd.optim import FusedAdamW
    opt = FusedAdamW(cpu_model.parameters(), lr=1e-3)   # the container needs no device; nothing is stepped here
    assert opt.ema is None
    ema = _StubEma()
    opt.attach_ema(ema)
    assert opt.ema is ema
    opt.note_replay()
    assert ema.dirty == 1          # a replayed step updated the average on the device
    opt.attach_ema(None)
    assert opt.ema is None
    opt.note_replay()
    assert ema.dirty == 1 and ema.calls == []
    with pytest.raises(TypeError):
        opt.attach_ema(object())
    assert opt.ema is None


def test_step_signatures_are_unchanged():
    """The lists of tests/test_train_step_api.py: the EMA rides on the optimizer object, no call gained a parameter."""
    from nvit_amd.optim import FusedAdamW
    from nvit_amd.train import GraphedTrainStep, train_step
    P, E = inspect.Parameter, inspect.Parameter.empty
    kinds = lambda fn: [(p.name, p.kind, p.default) for p in inspect.signature(fn).parameters.values()]
    tail = [("accumulation_steps", P.KEYWORD_ONLY, 1), ("skip_nonfinite", P.KEYWORD_ONLY, False)]
    assert kinds(train_step) == [
        ("model", P.POSITIONAL_OR_KEYWORD, E), ("optimizer", P.POSITIONAL_OR_KEYWORD, E),
        ("X", P.POSITIONAL_OR_KEYWORD, E), ("y", P.POSITIONAL_OR_KEYWORD, E),
        ("grad_clip", P.POSITIONAL_OR_KEYWORD, 1.0), ("sync_grads", P.POSITIONAL_OR_KEYWORD, None)] + tail
    assert kinds(GraphedTrainStep.__init__) == [
        ("self", P.POSITIONAL_OR_KEYWORD, E), ("model", P.POSITIONAL_OR_KEYWORD, E),
        ("optimizer", P.POSITIONAL_OR_KEYWORD, E), ("X", P.POSITIONAL_OR_KEYWORD, E), ("y", P.POSITIONAL_OR_KEYWORD, E),
        ("grad_clip", P.POSITIONAL_OR_KEYWORD, 1.0), ("warmup", P.POSITIONAL_OR_KEYWORD, 3)] + tail
    assert [(n, d) for n, _, d in kinds(FusedAdamW.step_fused)] == [
        ("self", E), ("model", None), ("grad_clip", 0.0), ("skip_nonfinite", False)]
    assert [n for n, _, _ in kinds(FusedAdamW.step)] == ["self", "closure"]
    assert [n for n, _, _ in kinds(FusedAdamW.attach_ema)] == ["self", "ema"]


def test_checkpoint_gains_exactly_one_key_and_loads_weights_only(cpu_model, tmp_path):
    from nvit_amd.checkpoint import build_checkpoint, load_checkpoint, save_checkpoint
    opt = cpu_model.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cpu")
    assert set(build_checkpoint(cpu_model, opt, 1, {})) == REF_KEYS
    assert set(build_checkpoint(cpu_model, opt, 1, {}, ema=None)) == REF_KEYS
    ema = _StubEma()
    assert set(build_checkpoint(cpu_model, opt, 1, {}, ema=ema)) == REF_KEYS | {"model_ema"}
    plain = save_checkpoint(tmp_path / "plain.pt", cpu_model, opt, 1, {"val/loss": 1.0})
    assert set(torch.load(plain, map_location="cpu", weights_only=False)) == REF_KEYS
    path = save_checkpoint(tmp_path / "ema.pt", cpu_model, opt, 1, {"val/loss": 1.0}, ema=ema)
    loaded = load_checkpoint(path, device="cpu", restore_rng=False)   # the default, weights-only load
    assert len(loaded) == 3
    ck = loaded[2]
    assert set(ck) == REF_KEYS | {"model_ema"}
    got, want = ck["model_ema"], ema.state_dict()
    assert set(got) == {"shadow", "updates", "decay", "warmup"}
    assert torch.equal(got["shadow"]["w"], want["shadow"]["w"])
    assert (got["updates"], got["decay"], got["warmup"]) == (3, 0.99, True)
    assert type(got["updates"]) is int and type(got["decay"]) is float and type(got["warmup"]) is bool


def test_decay_formula_against_a_hand_written_table():
    table = {   # (decay, t) -> d: (1 + t) / (10 + t) until it reaches the decay
        (0.9998, 0): 1.0 / 10.0, (0.9998, 1): 2.0 / 11.0, (0.9998, 9): 10.0 / 19.0, (0.9998, 10 ** 4): 10001.0 / 10010.0,
        (0.9, 0): 1.0 / 10.0, (0.9, 1): 2.0 / 11.0, (0.9, 9): 10.0 / 19.0, (0.9, 10 ** 4): 0.9,
    }
    for (decay, t), d in table.items():
        assert ema_ref.decay_at(t, decay, True) == d, (decay, t)
        assert ema_ref.decay_at(t, decay, False) == decay, (decay, t)
        assert ema_ref.omd_at(t, decay, True).dtype.name == "float32"
        assert float(ema_ref.omd_at(t, decay, True)) == pytest.approx(1.0 - d, rel=2.0 ** -24, abs=0.0)
    assert 0.99910 < table[(0.9998, 10 ** 4)] < 0.99911 and 0.52631 < table[(0.9998, 9)] < 0.52632
    # the warm-up reaches decay 0.9998 at (1 + t) / (10 + t) = 0.9998, t = 44990; 0.9 at t = 80
    assert ema_ref.decay_at(44988, 0.9998) < 0.9998 == ema_ref.decay_at(44992, 0.9998)
    assert ema_ref.decay_at(79, 0.9) < 0.9 == ema_ref.decay_at(81, 0.9)


def test_reference_recurrence_in_both_precisions():
    import numpy as np
    rng = np.random.default_rng(0)
    e0 = rng.standard_normal(1000).astype(np.float32)
    ws = [rng.standard_normal(1000).astype(np.float32) for _ in range(4)]
    omds = [ema_ref.omd_at(t, 0.9998) for t in range(4)]
    e64, e32 = ema_ref.recurrence(e0, ws, omds), ema_ref.recurrence(e0, ws, omds, np.float32)
    assert e64.dtype == np.float64 and e32.dtype == np.float32
    amp = np.max(np.abs(np.stack([e0] + ws)), axis=0)
    assert np.all(np.abs(e32 - e64) <= 4 * 2.0 ** -22 * amp)
    same = ema_ref.recurrence(e0, [e0] * 3, omds[:3], np.float32)
    assert same.tobytes() == e0.tobytes()          # p == e gives e back bit for bit
    assert np.all(np.abs(ema_ref.update32(e0, ws[0], omds[0]) - ema_ref.update64(e0, ws[0], omds[0]))
                  <= ema_ref.update_bound(e0, ws[0]))
