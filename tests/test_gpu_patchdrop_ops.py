"""GPU tests, op level, of patch dropout: nvit_patchdrop_draw against its numpy twin (patchdrop_ref.draw) bit for bit,
nvit_rows_gather against torch.index_select and ops.cast, nvit_rows_scatter against zeros.index_copy_, and the argument
checks of the wrappers.  Run on the MI355X box: pytest -m gpu."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import patchdrop_ref as pr

DEV = "cuda:0"
TIE_SEED = 1233   # patchdrop_ref.words(TIE_SEED, 0, 0, 64, 784) holds a tie of u across the cut at K = 392 (asserted below)


class _Keep:
    """a PatchDropout whose K is given, not derived from a rate"""

    def __new__(cls, K, seed=0, first_index=0):
        from nvit_amd import PatchDropout

        class Fixed(PatchDropout):
            def num_keep(self, T):
                return K

        return Fixed(0.5, seed=seed, first_index=first_index).to(DEV)


DRAW_SHAPES = [(1, 1, 1), (3, 16, 8), (5, 49, 24), (2, 49, 49), (64, 784, 392), (2, 4096, 1), (2, 4096, 4095)]


@pytest.mark.parametrize("B,T,K", DRAW_SHAPES)
def test_draw_equals_the_numpy_twin(B, T, K):
    seed, first = (TIE_SEED, 0) if T == 784 else (2 ** 63 + 12345, 2 ** 40 + 3)
    if T == 784:
        u = pr.words(seed, 0, first, B, T)
        key = np.sort((u << np.uint64(32)) | np.arange(T, dtype=np.uint64)[None, :], axis=1)
        assert ((key[:, 1:] >> np.uint64(32)) == (key[:, :-1] >> np.uint64(32))).any()   # a tie in u,
        assert ((key[:, K] >> np.uint64(32)) == (key[:, K - 1] >> np.uint64(32))).any()   # and one of them across the cut
    pd = _Keep(K, seed, first)
    for step in range(2):   # two consecutive calls: the counter advanced by exactly one each
        assert pd.step == step
        keep, slot = pd.draw(B, T)
        want_keep, want_slot = pr.draw(seed, step, first, B, T, K)
        assert keep.dtype == torch.int32 and tuple(keep.shape) == (B, K) and tuple(slot.shape) == (B, T)
        assert np.array_equal(keep.cpu().numpy(), want_keep)
        assert np.array_equal(slot.cpu().numpy(), want_slot)
    assert pd.step == 2


def test_draw_argument_checks():
    from nvit_amd import PatchDropout
    pd = PatchDropout(0.5).to(DEV)
    for B, T in ((0, 16), (-1, 16), (True, 16), (2.0, 16), (2, 0), (2, 4097), (2, 16.0), (2, True)):
        with pytest.raises(ValueError):
            pd.draw(B, T)
    assert pd.step == 0


def _rows(B, T, C, base):
    """fp32 [B*T, C] whose rows are all distinct: the row index (offset by `base`) in every element, plus the column / C"""
    r = torch.arange(B * T, dtype=torch.float32)[:, None] + base
    return (r + torch.arange(C, dtype=torch.float32)[None, :] / C).to(DEV).contiguous()


def _keep_table(B, T, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(T, generator=g)[:K].sort().values for _ in range(B)]).to(torch.int32)


ROW_SHAPES = [(1, 1, 1), (3, 16, 1), (5, 49, 24), (2, 784, 392), (3, 16, 16)]


@pytest.mark.parametrize("C", [64, 192, 768, 2048])
@pytest.mark.parametrize("B,T,K", ROW_SHAPES)
def test_gather_and_scatter_equal_torch(B, T, K, C):
    from nvit_amd import _lib, ops
    from nvit_amd._lib import BF16
    keep = _keep_table(B, T, K, 7 * B + T) if K < T else torch.arange(T, dtype=torch.int32).repeat(B, 1)
    slot = pr.slot_of(keep, T)
    flat = (keep.long() + torch.arange(B)[:, None] * T).reshape(-1).to(DEV)
    keep_d, slot_d = keep.to(DEV).contiguous(), slot.to(DEV).contiguous()
    s0, s1 = _rows(B, T, C, 0.0), _rows(B, T, C, 0.5)
    want0, want1 = s0.index_select(0, flat), s1.index_select(0, flat)
    for two in (True, False):
        for lo in (True, False):
            d0, d1, l0, l1 = ops.rows_gather(s0, s1 if two else None, keep_d, B, T, lo_dt=BF16 if lo else None)
            assert torch.equal(d0, want0) and (torch.equal(d1, want1) if two else d1 is None)
            if lo:
                assert torch.equal(l0, ops.cast(want0, BF16)) and l0.dtype == torch.bfloat16
                assert torch.equal(l1, ops.cast(want1, BF16)) if two else l1 is None
            else:
                assert l0 is None and l1 is None
    if K == T:
        assert torch.equal(want0, s0)   # the identity table
    # the backward: every element written (no NaN left from a dirty allocation), zeros at the dropped rows
    g0, g1 = _rows(B, K, C, 1.0), _rows(B, K, C, 1.5)
    z0 = torch.zeros(B * T, C, device=DEV).index_copy_(0, flat, g0)
    z1 = torch.zeros(B * T, C, device=DEV).index_copy_(0, flat, g1)
    for two in (True, False):
        o0, o1 = ops.rows_scatter(g0, g1 if two else None, slot_d, B, K)
        assert torch.equal(o0, z0) and (torch.equal(o1, z1) if two else o1 is None)
        # the entry point itself on destinations pre-filled with NaN
        n0, n1 = (torch.full((B * T, C), float("nan"), device=DEV) for _ in range(2))
        _lib.check(_lib.load().nvit_rows_scatter(ops._p(g0), ops._p(g1 if two else None), ops._p(slot_d), ops._p(n0),
                                                 ops._p(n1 if two else None), B, T, K, C, ops._s()), "nvit_rows_scatter")
        assert torch.equal(n0, z0) and (torch.equal(n1, z1) if two else bool(torch.isnan(n1).all()))


def test_wrappers_check_their_arguments_before_any_launch():
    from nvit_amd import ops
    from nvit_amd._lib import BF16, F32
    B, T, K, C = 2, 16, 8, 64
    s = _rows(B, T, C, 0.0)
    keep = _keep_table(B, T, K, 1).to(DEV)
    slot = pr.slot_of(keep.cpu(), T).to(DEV)
    d = _rows(B, K, C, 0.0)
    bad_gather = [
        dict(src0=s.cpu()), dict(src0=s.double()), dict(src0=s.t().contiguous().t()), dict(src0=s[:-1]),
        dict(src0=_rows(B, T, 66, 0.0)), dict(src1=s[:, :32].contiguous()), dict(src1=s.bfloat16()),
        dict(keep=keep.long()), dict(keep=keep.cpu()), dict(keep=keep[:1]), dict(keep=keep.reshape(-1)),
        dict(keep=torch.zeros(B, T + 1, dtype=torch.int32, device=DEV)), dict(B=3), dict(B=0), dict(T=7), dict(lo_dt=F32),
    ]
    for over in bad_gather:
        a = dict(src0=s, src1=s, keep=keep, B=B, T=T, lo_dt=BF16)
        a.update(over)
        with pytest.raises((ValueError, RuntimeError)):
            ops.rows_gather(a["src0"], a["src1"], a["keep"], a["B"], a["T"], lo_dt=a["lo_dt"])
    bad_scatter = [
        dict(d0=d.cpu()), dict(d0=d.bfloat16()), dict(d0=d[:-1]), dict(d1=d[:, :32].contiguous()), dict(slot=slot.long()),
        dict(slot=slot.cpu()), dict(slot=slot[:1]), dict(B=3), dict(K=K + 1), dict(K=0), dict(K=T + 1),
    ]
    for over in bad_scatter:
        a = dict(d0=d, d1=d, slot=slot, B=B, K=K)
        a.update(over)
        with pytest.raises((ValueError, RuntimeError)):
            ops.rows_scatter(a["d0"], a["d1"], a["slot"], a["B"], a["K"])
    # a hand-made table with an index outside [0, T) gathers zeros and scatters nothing from outside [0, K)
    wild = keep.clone()
    wild[0, 0], wild[1, 3] = -1, T
    d0, _, _, _ = ops.rows_gather(s, None, wild, B, T)
    assert (d0[0] == 0).all() and (d0[K + 3] == 0).all() and torch.equal(d0[1], s[int(wild[0, 1])])
    wslot = slot.clone()
    wslot[0, :] = K
    g0, _ = ops.rows_scatter(d, None, wslot, B, K)
    assert (g0[:T] == 0).all()
