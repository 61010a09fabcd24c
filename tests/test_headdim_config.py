"""Head dims the model accepts (no GPU): 32, 64 and 128; anything else is a ValueError.  In bf16 mode every accepted
head dim runs attention on the MFMA kernels (impl 1), in fp32 mode on the scalar-FMA kernels (impl 0)."""
import pytest

from nvit_amd.config import named_config
from nvit_amd.model import ViT


def test_head_dim_128_constructs():
    m = ViT(named_config("mini", n_embd=256, n_head=2))
    assert m.config.n_embd // m.config.n_head == 128


@pytest.mark.parametrize("n_embd,n_head", [(192, 4), (384, 4), (256, 16)])   # d = 48, 96, 16
def test_other_head_dims_raise(n_embd, n_head):
    with pytest.raises(ValueError, match="32, 64, 128"):
        ViT(named_config("mini", n_embd=n_embd, n_head=n_head))


@pytest.mark.parametrize("n_embd,n_head,d", [(128, 4, 32), (128, 2, 64), (256, 2, 128)])
def test_attn_impl_per_precision(n_embd, n_head, d):
    m = ViT(named_config("mini", n_embd=n_embd, n_head=n_head))
    assert m.config.n_embd // m.config.n_head == d
    assert m.set_precision("bf16")._attn_impl() == 1
    assert m.set_precision("fp32")._attn_impl() == 0
