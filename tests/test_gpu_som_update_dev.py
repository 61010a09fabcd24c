"""GPU: nvit_som_update_dev (the SOM update whose rate is read from device memory when the kernel runs) against
nvit_som_update (the rate by value).  Same launches and arithmetic, so for equal rates every comparison is bitwise; the
by-value entry itself is held to its fp64 bound in test_gpu_kohonen_ops.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 4, 1, 1), (3, 5, 20, 2, 2), (4, 16, 64, 3, 3), (8, 16, 64, 8, 8)]   # B, T, C, gm, gn
LA = float(np.float32(0.7 * 0.3))
LA2 = float(np.float32(0.05 * 0.9))


def _problem(B, T, C, gm, gn, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + T + C + gm)
    nodes = torch.randn(gm * gn, C, generator=g)
    x = torch.randn(B, T, C, generator=g)
    idx = torch.randint(0, gm * gn, (B * T,), generator=g)
    return nodes.cuda(), x.cuda(), idx.cuda(), (gm * gn) ** 0.5 / 2.0


def _by_value(nodes, x, idx, la, sigma, gm, gn, periodic):
    from nvit_amd import ops
    out = nodes.clone()
    B, T, _ = x.shape
    ops.som_update(out, x, idx, la, sigma, gm, gn, B, T, periodic=periodic)
    return out


@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("B,T,C,gm,gn", SHAPES)
def test_device_rate_gives_the_by_value_bits(B, T, C, gm, gn, periodic):
    from nvit_amd import ops
    nodes, x, idx, sigma = _problem(B, T, C, gm, gn)
    rate = torch.tensor([LA], device="cuda", dtype=torch.float32)
    want = _by_value(nodes, x, idx, LA, sigma, gm, gn, periodic)
    assert not torch.equal(want, nodes)
    got = nodes.clone()
    ops.som_update(got, x, idx, rate, sigma, gm, gn, B, T, periodic=periodic)
    assert torch.equal(got, want)
    # the rate is read when the kernel runs: another value in the same tensor gives that value's result
    rate.fill_(LA2)
    want2 = _by_value(nodes, x, idx, LA2, sigma, gm, gn, periodic)
    assert not torch.equal(want2, want)
    got2 = nodes.clone()
    ops.som_update(got2, x, idx, rate, sigma, gm, gn, B, T, periodic=periodic)
    assert torch.equal(got2, want2)
    # rate 0: node + 0 * (v - node), the nodes as they were
    rate.zero_()
    got0 = nodes.clone()
    ops.som_update(got0, x, idx, rate, sigma, gm, gn, B, T, periodic=periodic)
    assert torch.equal(got0, nodes)


def test_device_rate_on_a_side_stream():
    from nvit_amd import ops
    B, T, C, gm, gn = SHAPES[2]
    nodes, x, idx, sigma = _problem(B, T, C, gm, gn, seed=1)
    want = _by_value(nodes, x, idx, LA, sigma, gm, gn, True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rate = torch.tensor([LA], device="cuda", dtype=torch.float32)
        got = nodes.clone()
        ops.som_update(got, x, idx, rate, sigma, gm, gn, B, T, periodic=True)
    side.synchronize()
    assert torch.equal(got, want)


def test_rate_tensor_on_the_device_is_checked():
    from nvit_amd import ops
    nodes, x, idx, sigma = _problem(*SHAPES[1])
    for bad in (torch.tensor([LA]), torch.tensor([LA, LA], device="cuda"),
                torch.tensor([LA], device="cuda", dtype=torch.float64)):
        with pytest.raises(ValueError):
            ops.som_update(nodes, x, idx, bad, sigma, 2, 2, 3, 5)
