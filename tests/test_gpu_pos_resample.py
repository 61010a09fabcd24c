"""GPU tests, op level, of the position-embedding resampling kernels (nvit_pos_resample_fwd / bwd, ops.pos_resample_*,
nvit_amd.resample_pos_embed) against torch's fp64 F.interpolate(mode="bicubic", antialias=True, align_corners=False) and
its fp64 autograd, at a derived element bound; the adjoint identity on the kernels' own outputs; equal grids; two tables
in one launch.  One test runs on the CPU alone: it shows that the bound tells the target from its near relatives.
Run on the MI355X box: pytest -m gpu.

Element bound (pos_resample_ref.element_bound): (taps_y * taps_x + 3) * 2^-24 * sum |w_y| |w_x| |p|, one rounding per
product and per add, one for the product of the two weights, two for the fp32-rounded weights."""
import numpy as np
import pytest
import torch

import pos_resample_ref as ref
from nvit_amd import resample as R

gpu = pytest.mark.gpu
DEV = "cuda:0"
WIDTHS = [64, 192, 2048]
_DATA = {}


def table(g, C, seed=0):
    """Gaussian fp32 [g*g, C] (CPU), fixed per (g, C, seed)"""
    key = (g, C, seed)
    if key not in _DATA:
        _DATA[key] = torch.randn(g * g, C, generator=torch.Generator().manual_seed(1000 * g + C + seed))
    return _DATA[key]


def worst_ratio(got, want, bound):
    """max |got - want| / bound over the elements (an element with bound 0 must be exact)"""
    err = np.abs(got.astype(np.float64) - want)
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


# ------------------------------------------------------------------------------------------------ CPU: the bound rejects
@pytest.mark.parametrize("g,g2", ref.GRIDS)
def test_bound_accepts_fp32_and_rejects_other_operators(g, g2):
    """A plain fp32 evaluation of the tap table passes the bound with room; antialias=False, align_corners=True and the
    two grid axes swapped miss it by orders of magnitude (grid 1 excepted: every variant is the same constant)."""
    C = 16
    p = table(g, C).double()
    rows = R.host_tables(g, g2)[0]
    want = ref.target(p, g, g2).numpy()
    bound = ref.element_bound(rows, g, p.numpy())
    ok = worst_ratio(ref.fp32_evaluation(rows, g, p.numpy()), want, bound)
    print(f"[{g}->{g2}] fp32 evaluation at {ok:.2f} of the bound")
    assert ok <= 1.0
    if g == 1:
        return
    swapped = p.reshape(g, g, C).transpose(0, 1).reshape(g * g, C)
    wrong = {"antialias=False": ref.target(p, g, g2, antialias=False), "align_corners=True": ref.target(p, g, g2, align_corners=True),
             "axes swapped": ref.target(swapped, g, g2)}
    for name, t in wrong.items():
        r = worst_ratio(t.numpy(), want, bound)
        print(f"   {name}: {r:.1e} x the bound")
        assert r > 1e3, name


# ------------------------------------------------------------------------------------------------ GPU: forward
@gpu
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("g,g2", ref.GRIDS)
def test_forward_vs_fp64_interpolate(g, g2, C):
    from nvit_amd import ops
    p = table(g, C)
    out, none = ops.pos_resample_fwd(p.to(DEV), None, g, g2)
    assert none is None and out.dtype == torch.float32 and tuple(out.shape) == (g2 * g2, C)
    want = ref.target(p.double(), g, g2).numpy()
    bound = ref.element_bound(R.host_tables(g, g2)[0], g, p.double().numpy())
    r = worst_ratio(out.cpu().numpy(), want, bound)
    print(f"[fwd {g}->{g2} C={C}] worst error {r:.3f} of the bound")
    assert r <= 1.0


# ------------------------------------------------------------------------------------------------ GPU: backward
@gpu
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("g,g2", ref.GRIDS)
def test_backward_vs_fp64_autograd_and_adjoint_identity(g, g2, C):
    from nvit_amd import ops
    p, d = table(g, C), table(g2, C, seed=1)
    p64 = p.double().requires_grad_(True)
    ref.target(p64, g, g2).backward(d.double())
    fwd, bwd = R.host_tables(g, g2)
    got, none = ops.pos_resample_bwd(d.to(DEV), None, g, g2)
    assert none is None and got.dtype == torch.float32 and tuple(got.shape) == (g * g, C)
    bound_b = ref.element_bound(bwd, g2, d.double().numpy())
    r = worst_ratio(got.cpu().numpy(), p64.grad.numpy(), bound_b)
    print(f"[bwd {g}->{g2} C={C}] worst error {r:.3f} of the bound")
    assert r <= 1.0
    # <R p, d> = <p, R^T d> on the kernels' own outputs, in fp64: each side within its own elementwise bound
    out, _ = ops.pos_resample_fwd(p.to(DEV), None, g, g2)
    lhs = (out.cpu().double() * d.double()).sum().item()
    rhs = (p.double() * got.cpu().double()).sum().item()
    bound_f = ref.element_bound(fwd, g, p.double().numpy())
    slack = (bound_f * np.abs(d.double().numpy())).sum() + (bound_b * np.abs(p.double().numpy())).sum()
    print(f"   adjoint identity: |<Rp,d> - <p,R^T d>| = {abs(lhs - rhs):.3e}, allowed {slack:.3e}")
    assert abs(lhs - rhs) <= slack


@gpu
@pytest.mark.parametrize("g,g2", [(7, 4), (7, 10), (28, 36)])
def test_autograd_function_and_ranks(g, g2):
    import nvit_amd
    from nvit_amd import ops
    C = 192
    p = table(g, C).to(DEV)
    d = table(g2, C, seed=1).to(DEV)
    want_out, _ = ops.pos_resample_fwd(p, None, g, g2)
    want_grad, _ = ops.pos_resample_bwd(d, None, g, g2)
    for shape_in, shape_out in (((g * g, C), (g2 * g2, C)), ((1, g * g, C), (1, g2 * g2, C))):
        q = p.reshape(shape_in).clone().requires_grad_(True)
        out = nvit_amd.resample_pos_embed(q, g2)
        assert tuple(out.shape) == shape_out and out.requires_grad
        out.backward(d.reshape(shape_out))
        assert torch.equal(out.detach().reshape(g2 * g2, C), want_out)
        assert tuple(q.grad.shape) == shape_in and torch.equal(q.grad.reshape(g * g, C), want_grad)


# ------------------------------------------------------------------------------------------------ GPU: the no-op and the pair
@gpu
def test_equal_grids_return_the_input():
    import nvit_amd
    from nvit_amd import ops
    p, q = table(7, 64).to(DEV), table(7, 64, seed=1).to(DEV)
    a, b = ops.pos_resample_fwd(p, q, 7, 7)
    assert a is p and b is q
    a, b = ops.pos_resample_bwd(p, None, 7, 7)
    assert a is p and b is None
    assert nvit_amd.resample_pos_embed(p, 7) is p


@gpu
@pytest.mark.parametrize("g,g2,C", [(7, 4, 64), (7, 10, 192), (28, 36, 768), (14, 7, 2048)])
def test_two_tables_in_one_launch_equal_two_launches(g, g2, C):
    from nvit_amd import ops
    p, q = table(g, C).to(DEV), table(g, C, seed=2).to(DEV)
    a, b = ops.pos_resample_fwd(p, q, g, g2)
    assert torch.equal(a, ops.pos_resample_fwd(p, None, g, g2)[0]) and torch.equal(b, ops.pos_resample_fwd(q, None, g, g2)[0])
    d, e = table(g2, C, seed=1).to(DEV), table(g2, C, seed=3).to(DEV)
    ga, gb = ops.pos_resample_bwd(d, e, g, g2)
    assert torch.equal(ga, ops.pos_resample_bwd(d, None, g, g2)[0]) and torch.equal(gb, ops.pos_resample_bwd(e, None, g, g2)[0])


@gpu
def test_wrapper_argument_checks():
    from nvit_amd import ops
    p = table(7, 64).to(DEV)
    for bad in (p[:, :62].contiguous(), p[:48], p.double(), p.t(), torch.zeros(49, 4096, device=DEV)):
        with pytest.raises(ValueError):
            ops.pos_resample_fwd(bad, None, 7, 4)
    with pytest.raises(ValueError):
        ops.pos_resample_fwd(p, p[:, :32].contiguous(), 7, 4)
    with pytest.raises(ValueError, match="taps"):
        ops.pos_resample_fwd(p, None, 7, 64)
    with pytest.raises(ValueError):
        ops.pos_resample_bwd(p, None, 7, 4)    # the gradient of a 4 x 4 result has 16 rows
    with pytest.raises(RuntimeError):
        ops.pos_resample_fwd(table(7, 64), None, 7, 4)
