"""CPU: the evaluation API is exported, refuses a CPU-resident model like the model itself does, and the profiler
family of the gate-only SwiGLU GEMM sits at the end of the family table (the indices before it are an ABI)."""
import pytest
import torch


def _cpu_model():
    from nvit_amd.config import named_config
    from nvit_amd.model import ViT
    cfg = named_config("micro")
    return ViT(cfg), cfg


def test_evaluation_names_import_from_the_package():
    import nvit_amd
    from nvit_amd import estimate_loss, predict, validate
    from nvit_amd import evaluate
    assert predict is evaluate.predict and validate is evaluate.validate and estimate_loss is evaluate.estimate_loss
    assert callable(nvit_amd.predict)


def test_cpu_model_is_refused_with_the_models_own_error():
    from nvit_amd import estimate_loss, predict, validate
    m, cfg = _cpu_model()
    X = torch.zeros(2, cfg.channels, cfg.image_size, cfg.image_size)
    y = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError) as want:
        m._prepare(torch.device("cpu"))
    for call in (lambda: predict(m, X), lambda: validate(m, [(X, y)]), lambda: estimate_loss(m, [(X, y)], 1)):
        m.train()
        with pytest.raises(RuntimeError) as got:
            call()
        assert str(got.value) == str(want.value)
        assert m.training, "a refused call must leave the training flag alone"


def test_gate_only_gemm_family_is_appended():
    from nvit_amd import _lib
    assert _lib.KID_NAMES[0] == "gemm_nt" and _lib.KID_NAMES[-1] == "gemm_swiglu_act"
    assert _lib.KID_NAMES.index("gemm_swiglu") == 10
    lib = _lib.load()
    for i, name in enumerate(_lib.KID_NAMES):
        assert lib.nvit_prof_name(i) == name.encode()
    assert lib.nvit_prof_name(len(_lib.KID_NAMES)) == b"?"
