"""CPU: the public signature of the train step.  The options for gradient accumulation and for skipping a non-finite
step are keyword-only additions with defaults that change nothing; wrong values are refused with ValueError before any
device work, so the refusals can be checked on a CPU-resident model (which could not run a forward at all)."""
import inspect

import pytest
import torch

from nvit_amd.config import named_config


def _leading(sig, names):
    params = list(sig.parameters.values())[:len(names)]
    return [(p.name, p.kind, p.default) for p in params]


def test_train_step_leading_parameters_are_unchanged():
    from nvit_amd.train import train_step
    P, E = inspect.Parameter, inspect.Parameter.empty
    assert _leading(inspect.signature(train_step), range(6)) == [
        ("model", P.POSITIONAL_OR_KEYWORD, E), ("optimizer", P.POSITIONAL_OR_KEYWORD, E),
        ("X", P.POSITIONAL_OR_KEYWORD, E), ("y", P.POSITIONAL_OR_KEYWORD, E),
        ("grad_clip", P.POSITIONAL_OR_KEYWORD, 1.0), ("sync_grads", P.POSITIONAL_OR_KEYWORD, None)]


def test_new_parameters_are_keyword_only_with_neutral_defaults():
    from nvit_amd.optim import FusedAdamW
    from nvit_amd.train import GraphedTrainStep, train_step
    P = inspect.Parameter
    for fn, n_before in ((train_step, 6), (GraphedTrainStep.__init__, 7)):
        params = list(inspect.signature(fn).parameters.values())
        assert [(p.name, p.kind, p.default) for p in params[n_before:]] == [
            ("accumulation_steps", P.KEYWORD_ONLY, 1), ("skip_nonfinite", P.KEYWORD_ONLY, False)], fn
    g = list(inspect.signature(GraphedTrainStep.__init__).parameters.values())[1:7]
    assert [(p.name, p.default) for p in g][4:] == [("grad_clip", 1.0), ("warmup", 3)]
    s = list(inspect.signature(FusedAdamW.step_fused).parameters.values())
    assert [(p.name, p.default) for p in s[1:]] == [("model", None), ("grad_clip", 0.0), ("skip_nonfinite", False)]
    assert isinstance(FusedAdamW.skip_state, property) and callable(FusedAdamW.skipped_steps)


@pytest.fixture(scope="module")
def cpu_case():
    from nvit_amd.model import ViT
    cfg = named_config("micro")
    m = ViT(cfg)
    X = torch.zeros(8, cfg.channels, cfg.image_size, cfg.image_size)
    y = torch.zeros(8, dtype=torch.int64)
    return m, torch.optim.AdamW(m.parameters(), lr=1e-3), X, y


@pytest.mark.parametrize("n", [0, 1.5, 3])
def test_bad_accumulation_steps_raise_value_error_before_device_work(cpu_case, n):
    from nvit_amd.train import train_step
    m, opt, X, y = cpu_case
    step0 = m.step
    with pytest.raises(ValueError):
        train_step(m, opt, X, y, accumulation_steps=n)
    assert m.step == step0   # not even the forward's counter moved


def test_skip_nonfinite_needs_the_fused_optimizer(cpu_case):
    from nvit_amd.train import train_step
    m, opt, X, y = cpu_case
    with pytest.raises(ValueError):
        train_step(m, opt, X, y, skip_nonfinite=True)
