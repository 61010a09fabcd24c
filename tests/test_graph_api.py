"""CPU: the interface of the graph-replay features - GraphedTrainStep and GraphedEval are exported, the device-rate SOM
update entry is bound and exported, GraphedEval refuses a CPU-resident model before it changes anything, and
ops.som_update refuses a rate tensor that is not one fp32 element on the device.  No compute calls."""
import ctypes

import pytest
import torch


def test_graphed_classes_are_exported():
    from nvit_amd import GraphedEval, GraphedTrainStep
    from nvit_amd import evaluate, train
    assert GraphedTrainStep is train.GraphedTrainStep and GraphedEval is evaluate.GraphedEval
    for name in ("predict", "validate", "estimate_loss"):
        assert callable(getattr(GraphedEval, name)), name


def test_som_update_dev_is_bound_and_exported():
    from nvit_amd import _lib
    sig = _lib.SIGNATURES["nvit_som_update_dev"]
    assert len(sig) == 14
    # nvit_som_update's arguments with the rate as a pointer
    val = _lib.SIGNATURES["nvit_som_update"]
    assert sig[:3] == val[:3] and sig[3] is ctypes.c_void_p and val[3] is ctypes.c_float and sig[4:] == val[4:]
    assert hasattr(_lib.load(), "nvit_som_update_dev")


def test_graphed_eval_refuses_a_cpu_model_and_leaves_it_alone():
    from nvit_amd import GraphedEval
    from nvit_amd.config import named_config
    from nvit_amd.model import ViT
    m = ViT(named_config("micro_k"))
    X, y = torch.zeros(2, 3, 32, 32), torch.zeros(2, dtype=torch.int64)
    try:
        m._prepare(torch.device("cpu"))
    except RuntimeError as e:
        want = str(e)
    for flag in (True, False):
        m.train(flag)
        with pytest.raises(RuntimeError) as ei:
            GraphedEval(m, X, y)
        assert str(ei.value) == want
        assert m.training is flag and m.step == 0


@pytest.mark.parametrize("rate", [torch.tensor([0.21]), torch.tensor([0.21, 0.21]),
                                  torch.tensor([0.21], dtype=torch.float64)],
                         ids=["cpu", "two_elements", "fp64"])
def test_som_update_refuses_a_bad_rate_tensor(rate):
    from nvit_amd import ops
    nodes, x, idx = torch.zeros(4, 4), torch.zeros(1, 1, 4), torch.zeros(1, dtype=torch.int64)
    if torch.cuda.is_available():   # the shape and dtype cases on the device, where only they are wrong
        nodes, x, idx = nodes.cuda(), x.cuda(), idx.cuda()
        if rate.numel() != 1 or rate.dtype != torch.float32:
            rate = rate.cuda()
    before = nodes.clone()
    with pytest.raises(ValueError):
        ops.som_update(nodes, x, idx, rate, 1.0, 2, 2, 1, 1)
    assert torch.equal(nodes, before)
