"""CPU: the public face of patch dropout (nvit_amd.PatchDropout, ViT.attach_patch_drop, the checkpoint key) and the numpy
restatement of its draw (patchdrop_ref.py) that the GPU tests hold the kernel to bit for bit.  No device work."""
import numpy as np
import pytest
import torch

import patchdrop_ref as pr


def test_constructor_validation():
    from nvit_amd import PatchDropout
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            PatchDropout(bad)
    for bad in ("0.5", None, True, [0.5]):
        with pytest.raises(TypeError):
            PatchDropout(bad)
    with pytest.raises(ValueError):
        PatchDropout(0.5, seed=-1)
    with pytest.raises(ValueError):
        PatchDropout(0.5, seed=2 ** 64)
    with pytest.raises(TypeError):
        PatchDropout(0.5, seed=1.5)
    with pytest.raises(ValueError):
        PatchDropout(0.5, first_index=-1)
    with pytest.raises(ValueError):
        PatchDropout(0.5, first_index=2 ** 62)
    with pytest.raises(TypeError):
        PatchDropout(0.5, first_index=True)
    pd = PatchDropout(0)
    assert pd.rate == 0.0 and type(pd.rate) is float and pd.step == 0
    assert PatchDropout(0.25, seed=2 ** 64 - 1, first_index=2 ** 62 - 1).first_index == 2 ** 62 - 1
    with pytest.raises(RuntimeError):
        PatchDropout(0.5).draw(2, 16)          # no device yet
    with pytest.raises(RuntimeError):
        PatchDropout(0.5).to("cpu")


def test_num_keep_is_timms():
    from nvit_amd import PatchDropout
    from nvit_amd.patchdrop import MAX_TOKENS
    assert MAX_TOKENS == pr.MAX_TOKENS == 4096
    for rate in (0.0, 0.25, 0.5, 0.9):
        pd = PatchDropout(rate)
        for T in (1, 16, 49, 784):
            want = max(1, int(T * (1. - rate)))          # timm.layers.PatchDropout.forward
            assert pd.num_keep(T) == want == pr.num_keep(T, rate) and 1 <= want <= T
    assert [PatchDropout(0.5).num_keep(T) for T in (1, 16, 49, 784)] == [1, 8, 24, 392]
    assert PatchDropout(0.9).num_keep(1) == 1 and PatchDropout(0.0).num_keep(784) == 784
    for bad in (0, -1, 16.0, True):
        with pytest.raises(ValueError):
            PatchDropout(0.5).num_keep(bad)


def test_twin_properties():
    for seed, step, first, B, T, K in ((0, 0, 0, 4, 16, 8), (2 ** 63 + 11, 2 ** 33 + 5, 2 ** 40, 3, 49, 24),
                                       (5, 1, 0, 2, 49, 49), (5, 1, 0, 2, 50, 1), (9, 0, 7, 2, 1, 1)):
        keep, slot = pr.draw(seed, step, first, B, T, K)
        assert keep.dtype == np.int32 and slot.dtype == np.int32 and keep.shape == (B, K) and slot.shape == (B, T)
        assert (keep >= 0).all() and (keep < T).all()
        assert (np.diff(keep, axis=1) > 0).all()                            # exactly K distinct tokens, ascending
        assert ((slot >= 0).sum(axis=1) == K).all()
        for b in range(B):
            assert np.array_equal(slot[b, keep[b]], np.arange(K))           # slot is the inverse,
            assert (np.delete(slot[b], keep[b]) == -1).all()                # -1 everywhere else
        if K < T:
            assert not np.array_equal(pr.draw(seed, step + 1, first, B, T, K)[0], keep)    # another step,
            assert not np.array_equal(pr.draw(seed + 1, step, first, B, T, K)[0], keep)    # another seed
        # the kept set is the K smallest composite keys
        u = pr.words(seed, step, first, B, T)
        key = (u << np.uint64(32)) | np.arange(T, dtype=np.uint64)[None, :]
        assert (u < 2 ** 24).all()
        for b in range(B):
            assert set(keep[b]) == set(np.argsort(key[b])[:K])
    # a sample's draw depends on its global index only: a batch drawn in two halves is the batch
    whole = pr.draw(3, 9, 0, 8, 49, 24)
    half = pr.draw(3, 9, 4, 4, 49, 24)
    assert np.array_equal(whole[0][4:], half[0]) and np.array_equal(whole[1][4:], half[1])
    assert not np.array_equal(whole[0][:4], half[0])


def test_twin_keeps_every_token_equally_often():
    """T = 16, K = 8 over 20 480 samples: the keep frequency of every token lies within 5 standard deviations of K / T
    (the tie bias towards a low t is O(T / 2^24), far below this resolution)."""
    n, T, K = 20480, 16, 8
    keep, slot = pr.draw(17, 3, 0, n, T, K)
    f = (slot >= 0).mean(axis=0)
    sd = np.sqrt((K / T) * (1 - K / T) / n)
    assert f.shape == (T,) and (np.abs(f - K / T) <= 5 * sd).all(), (f, sd)


def test_tie_goes_to_the_smaller_token():
    """(seed 1233, step 0, B = 64, T = 784): sample 22 holds two tokens with the same word u that the cut at K = 392
    separates - found with the twin, asserted here before it is used; the smaller t is the one kept."""
    seed, B, T, K = 1233, 64, 784, 392
    u = pr.words(seed, 0, 0, B, T)
    keep, slot = pr.draw(seed, 0, 0, B, T, K)
    cases = []
    for b in range(B):
        kept = slot[b] >= 0
        worst_kept = u[b][kept].max()
        best_dropped = u[b][~kept].min()
        assert worst_kept <= best_dropped
        if worst_kept == best_dropped:
            cases.append((b, np.nonzero(kept & (u[b] == worst_kept))[0], np.nonzero(~kept & (u[b] == worst_kept))[0]))
    assert cases, "no sample of this draw has a tie across the cut"
    for b, t_kept, t_dropped in cases:
        assert len(t_kept) >= 1 and len(t_dropped) >= 1 and t_kept.max() < t_dropped.min(), (b, t_kept, t_dropped)


def test_state_dict_round_trip(tmp_path):
    from nvit_amd import PatchDropout
    pd = PatchDropout(0.5, seed=2 ** 40 + 7)
    pd.load_state_dict({"seed": 2 ** 63 + 5, "step": 123456789012})
    assert pd.state_dict() == {"seed": 2 ** 63 + 5, "step": 123456789012}
    torch.save(pd.state_dict(), tmp_path / "pd.pt")
    other = PatchDropout(0.5)
    other.load_state_dict(torch.load(tmp_path / "pd.pt", weights_only=True))
    assert other.state_dict() == pd.state_dict() and other.step == 123456789012
    with pytest.raises(ValueError):
        other.load_state_dict({"seed": 1, "step": -1})


def test_checkpoint_key_set():
    from nvit_amd import DropPath, PatchDropout, ViT, named_config
    from nvit_amd.checkpoint import build_checkpoint
    m = ViT(named_config("micro"))
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    base = build_checkpoint(m, opt, 3, {"loss": 1.0})
    assert "patch_drop" not in base
    pd = PatchDropout(0.5, seed=5)
    pd.load_state_dict({"seed": 5, "step": 42})
    ck = build_checkpoint(m, opt, 3, {"loss": 1.0}, patch_drop=pd)
    assert set(ck) == set(base) | {"patch_drop"} and ck["patch_drop"] == {"seed": 5, "step": 42}
    both = build_checkpoint(m, opt, 3, {"loss": 1.0}, patch_drop=pd, drop_path=DropPath(0.1))
    assert set(both) == set(base) | {"patch_drop", "drop_path"}


def test_attach_patch_drop():
    from nvit_amd import DropPath, PatchDropout, ViT, named_config
    m = ViT(named_config("micro"))
    assert m.patch_drop is None
    pd = PatchDropout(0.5)
    assert m.attach_patch_drop(pd) is m and m.patch_drop is pd
    assert "patch_drop" not in "".join(m.state_dict().keys())
    m.attach_drop_path(DropPath(0.1))                     # the two go together
    assert m.patch_drop is pd and m.drop_path is not None
    m.attach_patch_drop(None)
    assert m.patch_drop is None
    for bad in (0.5, "pd", DropPath(0.1)):
        with pytest.raises(TypeError):
            m.attach_patch_drop(bad)
    assert m.patch_drop is None
    for name in ("micro_vit", "micro_fa", "hd80"):       # plain ViT, flash_attn=True, padded heads
        assert ViT(named_config(name)).attach_patch_drop(PatchDropout(0.25)).patch_drop is not None
    with pytest.raises(ValueError):
        ViT(named_config("micro_k")).attach_patch_drop(pd)
    from dataclasses import fields
    from nvit_amd import ViTConfig
    assert not any("patch_drop" in f.name for f in fields(ViTConfig))


def test_restatements_with_every_token_kept_are_the_oracles():
    """patchdrop_ref's forwards with the identity table restate the unchanged oracles: the nViT one equals
    oracle.nvit_oracle's logits and gradients bit for bit in fp64, the plain one vit_torch_ref's to fp64 round-off; a real
    subset differs."""
    import vit_torch_ref
    from nvit_amd import named_config
    from nvit_amd.weights import formula_state_dict, synthetic_batch
    from oracle import nvit_oracle as O
    cfg = named_config("micro")
    B, T = 4, 16
    X, y = synthetic_batch(cfg, B)
    ident = torch.arange(T, dtype=torch.int32).repeat(B, 1)
    p0 = {n: t.detach().clone().double().requires_grad_(True) for n, t in formula_state_dict(cfg).items()}
    logits0, _, _ = O.loss_and_grads(p0, cfg, X.double(), y)
    p1, logits1, _ = pr.dropped_loss_and_grads(formula_state_dict(cfg), cfg, X, y, ident)
    assert torch.equal(logits0, logits1)
    for n, t in p0.items():
        if n.startswith("reconstruction_head"):
            assert p1[n].grad is None          # the dropping forward leaves the head out
        else:
            assert (t.grad is None) == (p1[n].grad is None) and (t.grad is None or torch.equal(t.grad, p1[n].grad)), n
    keep = torch.tensor([[0, 3, 4, 9, 10, 11, 14, 15], [1, 2, 3, 4, 5, 6, 7, 8], [0, 2, 4, 6, 8, 10, 12, 14],
                         [1, 3, 5, 7, 9, 11, 13, 15]], dtype=torch.int32)
    assert torch.equal(pr.slot_of(keep, T)[0, keep[0].long()], torch.arange(8, dtype=torch.int32))
    _, logits2, _ = pr.dropped_loss_and_grads(formula_state_dict(cfg), cfg, X, y, keep)
    assert (logits2 - logits0).abs().max().item() > 1e-3
    cfg = named_config("micro_vit")
    sd = formula_state_dict(cfg)
    l0, _, _, g0 = vit_torch_ref.loss_and_grads(sd, cfg, X, y)
    l1, _, g1 = pr.dropped_vit_loss_and_grads(sd, cfg, X, y, ident)
    # (the gather returns a contiguous copy where vit_torch_ref goes on with a transposed view: fp64 round-off, not bits)
    assert (l0 - l1).abs().max().item() < 1e-13 and set(g0) == set(g1)
    for k in g1:
        assert (g0[k] - g1[k]).abs().max().item() <= 1e-12 * g0[k].abs().max().item() + 1e-18, k
    l2, _, g2 = pr.dropped_vit_loss_and_grads(sd, cfg, X, y, keep)
    assert (l2 - l0).abs().max().item() > 1e-5          # (far above the 1e-13 of the identity table)
    # position-embedding rows of tokens nobody kept get no gradient
    dropped = sorted(set(range(T)) - set(keep.flatten().tolist()))
    assert dropped == [] or (g2["local_pos_embed"][0, dropped] == 0).all()
