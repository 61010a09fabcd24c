"""GPU tests, model level, of patch dropout (ViT.attach_patch_drop): a fixed table of kept tokens (a PatchDropout whose
`draw` is overridden) through the whole forward and backward - the identity table against the model with nothing attached
bit for bit, a real subset against the fp64 restatement built from the CPU oracle's own pieces (patchdrop_ref) at the bars
test_gpu_droppath.py holds the same models to; the gradient rows of tokens nobody kept; the drawn tables against the numpy
twin through three train steps; the captured train step against eager steps bit for bit; resume from a checkpoint; and
what the feature must not change (eval, predict, validate).  Run on the MI355X box: pytest -m gpu."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import patchdrop_ref as pr
from nvit_amd.config import named_config
from nvit_amd.weights import formula_state_dict, synthetic_batch

DEV = "cuda:0"


def build(cfg, precision, renormed=False):
    from nvit_amd.model import ViT
    from nvit_amd.train import normalize_matrices
    m = ViT(cfg)
    m.load_state_dict(formula_state_dict(cfg), strict=False)
    m = m.to(DEV).set_precision(precision)
    if renormed:
        normalize_matrices(m)
    return m


def fixed_patch_drop(tables):
    """a PatchDropout whose draws are the given keep tables [B, K], one per call (the last one again after that)"""
    from nvit_amd import PatchDropout
    tables = [tables] if isinstance(tables, torch.Tensor) else list(tables)

    class Fixed(PatchDropout):
        calls = 0

        def draw(self, B, T):
            keep = tables[min(Fixed.calls, len(tables) - 1)]
            Fixed.calls += 1
            assert keep.shape[0] == B and keep.shape[1] <= T
            return keep.to(DEV).contiguous(), pr.slot_of(keep, T).to(DEV).contiguous()

    return Fixed(0.5), Fixed


def keep_table(B, T, K, seed, never=()):
    """[B, K] int32, ascending per sample, another subset for every sample; the tokens `never` are kept by nobody"""
    g = torch.Generator().manual_seed(seed)
    pool = torch.tensor([t for t in range(T) if t not in never])
    rows = [pool[torch.randperm(len(pool), generator=g)[:K]].sort().values for _ in range(B)]
    keep = torch.stack(rows).to(torch.int32)
    assert all(not torch.equal(rows[b], rows[(b + 1) % B]) for b in range(B))
    return keep


def n_tokens(cfg):
    return (cfg.image_size // cfg.local_patch_size) ** 2


# ---------------------------------------------------------------------------------------------- identity
@pytest.mark.parametrize("name,precision", [("mini", "fp32"), ("mini", "bf16"), ("mini_vit", "fp32"), ("mini_vit", "bf16"),
                                            ("micro_fa", "fp32"), ("micro_fa", "bf16")])
def test_keeping_every_token_changes_no_bit(name, precision):
    from nvit_amd.train import total_loss
    cfg = named_config(name)
    B, T = 4, n_tokens(cfg)
    X, y = synthetic_batch(cfg, B)
    X, y = X.to(DEV), y.to(DEV)
    plain = build(cfg, precision).train()
    logits0, aux0 = plain(X)
    loss0 = total_loss(cfg, logits0, aux0, y)
    loss0.backward()
    m = build(cfg, precision).train()
    pd, Fixed = fixed_patch_drop(torch.arange(T, dtype=torch.int32).repeat(B, 1))
    m.attach_patch_drop(pd)
    logits, aux = m(X)
    assert Fixed.calls == 1                                            # one draw per training forward
    loss = total_loss(cfg, logits, aux, y)
    loss.backward()
    assert torch.equal(logits, logits0) and torch.equal(loss, loss0)
    assert set(aux0) - set(aux) == {"reconstruction"} and set(aux) <= set(aux0)
    for (n, p0), (_, p) in zip(plain.named_parameters(), m.named_parameters()):
        assert (p0.grad is None) == (p.grad is None), n
        assert p.grad is None or torch.equal(p0.grad, p.grad), n
    assert m._rt.tokens is None                                        # the forward left no token count behind


# ---------------------------------------------------------------------------------------------- against the restatement
# The bars of tests/test_gpu_droppath.py for these models: nViT fp32 logits and loss 1e-5, every gradient 2e-4 of its
# largest element (+ 1e-8); nViT bf16 logits 1e-3 against the oracle on renormalised weights; plain ViT fp32 logits 1e-5 of
# their largest, gradients 2e-4, bf16 logits 1e-2.
CASES = [("mini", 4, 24), ("micro", 8, 8), ("hd80", 4, 24)]
_REF = {}


def reference(name, B, K, renormed):
    """(keep, params with fp64 gradients, logits, loss), computed once per case"""
    key = (name, B, K, renormed)
    if key not in _REF:
        torch.set_num_threads(8)
        cfg = named_config(name)
        keep = keep_table(B, n_tokens(cfg), K, 11)
        X, y = synthetic_batch(cfg, B)
        _REF[key] = (keep,) + pr.dropped_loss_and_grads(formula_state_dict(cfg), cfg, X, y, keep, renormed=renormed)
    return _REF[key]


@pytest.mark.parametrize("name,B,K", CASES)
def test_fp32_dropped_forward_backward_vs_fp64_restatement(name, B, K):
    from nvit_amd.train import total_loss
    cfg = named_config(name)
    X, y = synthetic_batch(cfg, B)
    keep, p, logits_ref, loss_ref = reference(name, B, K, False)
    m = build(cfg, "fp32").train()
    m.attach_patch_drop(fixed_patch_drop(keep)[0])
    logits, aux = m(X.to(DEV))
    assert "reconstruction" not in aux
    loss = total_loss(cfg, logits, aux, y.to(DEV))
    loss.backward()
    err = (logits.detach().double().cpu() - logits_ref).abs().max().item()
    print(f"[fp32 dropped {name} K={K}] max|dlogit|={err:.3e} loss {loss.item():.6f} vs {loss_ref.item():.6f}")
    worst = 0.0
    have = {n for n, q in m.named_parameters() if q.grad is not None}
    want = {n for n, t in p.items() if t.grad is not None}
    for n in have & want:
        ref = p[n].grad
        e, s = (dict(m.named_parameters())[n].grad.double().cpu() - ref).abs().max().item(), ref.abs().max().item()
        worst = max(worst, e / (s + 1e-12))
    print(f"   worst relative grad error {worst:.3e}")
    assert err < 1e-5
    assert abs(loss.item() - loss_ref.item()) < 1e-5
    assert have == want, have ^ want
    for n, q in m.named_parameters():
        if q.grad is not None:
            ref = p[n].grad
            e, s = (q.grad.double().cpu() - ref).abs().max().item(), ref.abs().max().item()
            assert e <= 2e-4 * s + 1e-8, (n, e, s)
    # sample b run with sample b+1's indices is another function: it misses the bar
    shifted = build(cfg, "fp32").train()
    shifted.attach_patch_drop(fixed_patch_drop(torch.roll(keep, -1, 0))[0])
    ls, _ = shifted(X.to(DEV))
    err_s = (ls.detach().double().cpu() - logits_ref).abs().max().item()
    print(f"   table shifted by one sample: max|dlogit|={err_s:.3e}")
    assert err_s >= 1e-5


@pytest.mark.parametrize("name,B,K", CASES)
def test_bf16_dropped_forward_vs_fp64_restatement(name, B, K):
    from nvit_amd.train import total_loss
    cfg = named_config(name)
    X, y = synthetic_batch(cfg, B)
    keep, p, logits_ref, _ = reference(name, B, K, True)
    m = build(cfg, "bf16", renormed=True).train()
    m.attach_patch_drop(fixed_patch_drop(keep)[0])
    logits, aux = m(X.to(DEV))
    total_loss(cfg, logits, aux, y.to(DEV)).backward()
    err = (logits.detach().double().cpu() - logits_ref).abs().max().item()
    shifted = build(cfg, "bf16", renormed=True).train()
    shifted.attach_patch_drop(fixed_patch_drop(torch.roll(keep, -1, 0))[0])
    ls, _ = shifted(X.to(DEV))
    err_s = (ls.detach().double().cpu() - logits_ref).abs().max().item()
    print(f"[bf16 dropped {name} K={K}] max|dlogit| vs the fp64 restatement {err:.3e}; table shifted by one sample {err_s:.3e}")
    assert err < 1e-3
    assert err_s >= 1e-3
    have = {n for n, q in m.named_parameters() if q.grad is not None}
    assert have == {n for n, t in p.items() if t.grad is not None}
    for n, q in m.named_parameters():
        assert q.grad is None or torch.isfinite(q.grad).all(), n


def test_plain_vit_dropped_forward_backward_vs_fp64_restatement():
    cfg = named_config("mini_vit")
    B, K = 4, 24
    X, y = synthetic_batch(cfg, B)
    keep = keep_table(B, n_tokens(cfg), K, 11)
    ref_logits, _, ref_grads = pr.dropped_vit_loss_and_grads(formula_state_dict(cfg), cfg, X, y, keep)
    m = build(cfg, "fp32").train()
    m.attach_patch_drop(fixed_patch_drop(keep)[0])
    logits, aux = m(X.to(DEV))
    assert "reconstruction" not in aux
    torch.nn.functional.cross_entropy(logits, y.to(DEV)).backward()
    e, s_ = (logits.detach().double().cpu() - ref_logits).abs().max().item(), ref_logits.abs().max().item()
    worst = 0.0
    for n, q in m.named_parameters():
        if n in ref_grads and q.grad is not None and ref_grads[n].abs().max().item() > 1e-6:   # (the 1e-8 floor of the bar)
            worst = max(worst, (q.grad.double().cpu() - ref_grads[n]).abs().max().item()
                        / ref_grads[n].abs().max().item())
    print(f"[fp32 dropped mini_vit K={K}] max|dlogit| {e:.3e} of {s_:.3f}; worst relative grad error {worst:.3e}")
    assert e <= 1e-5 * s_ + 1e-12
    for n, q in m.named_parameters():
        if n in ref_grads:
            r = ref_grads[n]
            assert (q.grad.double().cpu() - r).abs().max().item() <= 2e-4 * r.abs().max().item() + 1e-8, n
        else:
            assert q.grad is None, n
    shifted = build(cfg, "fp32").train()
    shifted.attach_patch_drop(fixed_patch_drop(torch.roll(keep, -1, 0))[0])
    ls, _ = shifted(X.to(DEV))
    e_s = (ls.detach().double().cpu() - ref_logits).abs().max().item()
    print(f"   table shifted by one sample: max|dlogit| {e_s:.3e}")
    assert e_s > 1e-5 * s_ + 1e-12
    mb = build(cfg, "bf16").train()
    mb.attach_patch_drop(fixed_patch_drop(keep)[0])
    lb, _ = mb(X.to(DEV))
    torch.nn.functional.cross_entropy(lb, y.to(DEV)).backward()
    eb = (lb.detach().double().cpu() - ref_logits).abs().max().item()
    print(f"[bf16 dropped mini_vit] max|dlogit| {eb:.3e}")
    assert torch.isfinite(lb).all() and eb < 1e-2
    for n, q in mb.named_parameters():
        assert (q.grad is not None) == (n in ref_grads) and (q.grad is None or torch.isfinite(q.grad).all()), n


@pytest.mark.parametrize("name,precision", [("mini", "fp32"), ("mini", "bf16"), ("mini_vit", "bf16")])
def test_position_embedding_rows_of_tokens_nobody_kept_get_zero_gradient(name, precision):
    cfg = named_config(name)
    B, T, K = 4, n_tokens(cfg), 24
    never = (0, 7, 30, 48)
    keep = keep_table(B, T, K, 5, never=never)
    X, y = synthetic_batch(cfg, B)
    m = build(cfg, precision).train()
    m.attach_patch_drop(fixed_patch_drop(keep)[0])
    logits, _ = m(X.to(DEV))
    torch.nn.functional.cross_entropy(logits, y.to(DEV)).backward()
    dropped = sorted(set(range(T)) - set(keep.flatten().tolist()))
    assert set(never) <= set(dropped)
    kept = sorted(set(keep.flatten().tolist()))
    for g in (m.local_pos_embed.grad, m.global_pos_embed.grad):
        assert tuple(g.shape) == (1, T, cfg.n_embd)
        assert (g[0, dropped] == 0).all()
        assert (g[0, kept].abs().amax(dim=1) > 0).all()


# ---------------------------------------------------------------------------------------------- the draw inside the model
def same_weights(a, b):
    for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(pa, pb), n


def test_drawn_tables_are_the_twins():
    """3 train steps with the real draw = 3 steps whose tables come from the numpy twin at (seed, step)"""
    from nvit_amd import PatchDropout
    from nvit_amd.train import train_step
    cfg = named_config("mini")
    B, T = 4, n_tokens(cfg)
    X, y = synthetic_batch(cfg, B)
    X, y = X.to(DEV), y.to(DEV)
    seed, first = 2 ** 40 + 9, 12
    pd = PatchDropout(0.5, seed=seed, first_index=first).to(DEV)
    K = pd.num_keep(T)
    assert K == 24
    ma, mb = build(cfg, "fp32").train(), build(cfg, "fp32").train()
    ma.attach_patch_drop(pd)
    twins = [torch.from_numpy(pr.draw(seed, s, first, B, T, K)[0]) for s in range(3)]
    assert not torch.equal(twins[0], twins[1])
    fixed, Fixed = fixed_patch_drop(twins)
    mb.attach_patch_drop(fixed)
    oa = ma.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    ob = mb.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    for i in range(3):
        la, lossa, _, _ = train_step(ma, oa, X, y)
        lb, lossb, _, _ = train_step(mb, ob, X, y)
        assert torch.equal(la, lb) and torch.equal(lossa, lossb), i
        assert pd.step == i + 1
    assert Fixed.calls == 3
    same_weights(ma, mb)


@pytest.mark.parametrize("accum,with_drop_path", [(1, False), (2, False), (1, True)])
def test_graphed_train_step_with_patch_drop_equals_eager(accum, with_drop_path):
    """4 calls on the graphed model - replay, eager step, replay, replay - = 4 eager steps from the same state: logits,
    loss, weights, optimizer state and the counters bit for bit; accumulation_steps = 2 advances the counter by 2 per call
    and equals the hand-written loop; together with an attached DropPath; another PatchDropout at replay is refused."""
    from nvit_amd import DropPath, PatchDropout
    from nvit_amd.train import GraphedTrainStep, total_loss, train_step
    cfg = named_config("mini")
    B = 4
    X, y = synthetic_batch(cfg, B)
    X, y = X.to(DEV), y.to(DEV)
    X2, y2 = synthetic_batch(cfg, B, seed=77)
    X2, y2 = X2.to(DEV), y2.to(DEV)
    me, mg = build(cfg, "bf16", True).train(), build(cfg, "bf16", True).train()
    pe, pg = PatchDropout(0.5, seed=11).to(DEV), PatchDropout(0.5, seed=11).to(DEV)
    me.attach_patch_drop(pe)
    mg.attach_patch_drop(pg)
    if with_drop_path:
        de, dg = DropPath(0.3, seed=4).to(DEV), DropPath(0.3, seed=4).to(DEV)
        me.attach_drop_path(de)
        mg.attach_drop_path(dg)
    oe = me.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    og = mg.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    warm = 2
    for _ in range(warm):
        train_step(me, oe, X, y, accumulation_steps=accum)
    g = GraphedTrainStep(mg, og, X, y, warmup=warm, accumulation_steps=accum)
    assert pe.step == pg.step == warm * accum                           # the capture pass itself drew nothing
    for i, (xb, yb) in enumerate(((X, y), (X2, y2), (X, y), (X2, y2))):
        le, losse, _, gne = train_step(me, oe, xb, yb, accumulation_steps=accum)
        if i == 1:   # an eager step on the graphed model between two replays
            lg, lossg, _, gng = train_step(mg, og, xb, yb, accumulation_steps=accum)
        else:
            lg, lossg, _, gng = g(xb, yb)
        assert torch.equal(le, lg) and torch.equal(losse, lossg) and torch.equal(gne, gng), i
        assert pg.step == (warm + i + 1) * accum
    same_weights(me, mg)
    for (se, sg) in zip(oe.state_dict()["state"].values(), og.state_dict()["state"].values()):
        for k in se:
            assert torch.equal(torch.as_tensor(se[k]), torch.as_tensor(sg[k])), k
    assert pe.step == pg.step == (warm + 4) * accum
    if with_drop_path:
        assert de.step == dg.step == (warm + 4) * accum
    if accum == 2:
        # the hand-written loop, in lockstep from the same start: two half batches, each with its own draw, the losses
        # halved, one optimizer step
        mh = build(cfg, "bf16", True).train()
        ph = PatchDropout(0.5, seed=11).to(DEV)
        mh.attach_patch_drop(ph)
        oh = mh.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
        for xb, yb in ((X, y), (X, y), (X, y), (X2, y2), (X, y), (X2, y2)):
            for i in range(2):
                sl = slice(i * B // 2, (i + 1) * B // 2)
                lh, ah = mh(xb[sl])
                (total_loss(cfg, lh, ah, yb[sl]) / 2).backward()
            oh.step_fused(mh, 1.0)
            oh.zero_grad(set_to_none=True)
        assert ph.step == pe.step
        same_weights(me, mh)
    mg.attach_patch_drop(PatchDropout(0.5, seed=11).to(DEV))
    with pytest.raises(ValueError):
        g(X, y)
    mg.attach_patch_drop(None)
    with pytest.raises(ValueError):
        g(X, y)
    mg.attach_patch_drop(pg)
    g(X, y)


def test_resume_from_a_checkpoint(tmp_path):
    """save with patch_drop= after 2 steps, restore into fresh objects: step 3 has the uninterrupted run's bits"""
    from nvit_amd import PatchDropout
    from nvit_amd.checkpoint import load_checkpoint, save_checkpoint
    from nvit_amd.train import train_step
    cfg = named_config("mini")
    X, y = synthetic_batch(cfg, 4)
    X, y = X.to(DEV), y.to(DEV)
    m = build(cfg, "bf16", True).train()
    pd = PatchDropout(0.5, seed=21).to(DEV)
    m.attach_patch_drop(pd)
    opt = m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    for _ in range(2):
        train_step(m, opt, X, y)
    save_checkpoint(tmp_path / "ck.pt", m, opt, 2, {"loss": 0.0}, patch_drop=pd)
    want_logits, want_loss, _, _ = train_step(m, opt, X, y)
    m2, opt2, ck = load_checkpoint(tmp_path / "ck.pt", DEV,
                                   optimizer_factory=lambda mm: mm.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda"))
    assert ck["patch_drop"] == {"seed": 21, "step": 2}
    pd2 = PatchDropout(0.5).to(DEV)
    pd2.load_state_dict(ck["patch_drop"])
    m2 = m2.set_precision("bf16").train()
    m2.attach_patch_drop(pd2)
    got_logits, got_loss, _, _ = train_step(m2, opt2, X, y)
    assert torch.equal(got_logits, want_logits) and torch.equal(got_loss, want_loss)
    same_weights(m, m2)
    assert pd2.step == pd.step == 3


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_inactive_patch_drop_changes_no_bit(precision):
    """rate 0 attached in training mode; a live rate under eval(), torch.no_grad() in training mode, predict, validate and
    GraphedEval: the bits of the model with nothing attached, and no draw (the counter stays where it was)."""
    from nvit_amd import PatchDropout
    from nvit_amd.evaluate import GraphedEval, predict, validate
    cfg = named_config("mini")
    X, y = synthetic_batch(cfg, 4)
    X, y = X.to(DEV), y.to(DEV)
    plain = build(cfg, precision).train()
    want_train, aux_train = plain(X)
    with torch.no_grad():
        want_nograd, _ = plain(X)
    plain.eval()
    with torch.no_grad():
        want_eval, _ = plain(X)
    want_val = validate(plain, [(X, y)])
    m = build(cfg, precision).train()
    zero = PatchDropout(0.0).to(DEV)
    m.attach_patch_drop(zero)
    got, aux = m(X)
    assert torch.equal(got, want_train) and zero.step == 0 and set(aux) == set(aux_train)
    live = PatchDropout(0.5).to(DEV)
    m.attach_patch_drop(live)
    with torch.no_grad():
        got, _ = m(X)
    assert torch.equal(got, want_nograd)
    m.eval()
    with torch.no_grad():
        got, _ = m(X)
    assert torch.equal(got, want_eval)
    got, aux = m(X)                                   # eval mode with gradients enabled
    assert torch.equal(got, want_eval) and "reconstruction" in aux
    assert torch.equal(predict(m, X), want_eval)
    got_val = validate(m, [(X, y)])
    assert got_val == want_val
    ge = GraphedEval(m, X, y)
    assert torch.equal(ge.predict(X), want_eval)
    assert live.step == 0
    m.train()
    got, aux = m(X)
    assert live.step == 1 and not torch.equal(got, want_train) and "reconstruction" not in aux
