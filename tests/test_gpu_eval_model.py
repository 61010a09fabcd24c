"""GPU: the forward-only route of the model (torch.no_grad / inference_mode) and nvit_amd.evaluate.

The route must return the bits of the grad-enabled forward (that identity is what makes the switch automatic), must
actually be taken (profiler launch counts, peak memory), and validate / estimate_loss must report what the reference's
Trainer.validate / estimate_loss report (train.py:577-627, 482-506) without disturbing training."""
import pytest
import torch
import torch.nn.functional as F_

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def build(name, precision="bf16", train=False):
    from nvit_amd.config import named_config
    from nvit_amd.model import ViT
    from nvit_amd.weights import load_formula_weights
    cfg = named_config(name)
    m = ViT(cfg)
    load_formula_weights(m, cfg)
    m = m.to(DEV).set_precision(precision)
    return (m.train() if train else m.eval()), cfg


def batch(cfg, B, seed=1234):
    from nvit_amd.weights import synthetic_batch
    X, y = synthetic_batch(cfg, B, seed=seed)
    return X.to(DEV), y.to(DEV)


IDENTITY = [("micro", 8), ("micro_k", 8), ("mini", 4), ("tiny", 8), ("micro_vit", 8), ("micro_fa", 8), ("micro_k_fa", 8),
            ("base", 2)]


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("name,B", IDENTITY)
def test_no_grad_forward_is_the_grad_enabled_forward_bit_for_bit(name, B, precision):
    """Guards behaviour (bench.py's parity legs and smoke() call the forward under no_grad): passes without the
    forward-only route too."""
    from nvit_amd import predict
    m, cfg = build(name, precision)
    X, _ = batch(cfg, B)
    logits, aux = m(X)
    assert logits.requires_grad
    with torch.no_grad():
        l0, a0 = m(X)
    with torch.inference_mode():
        l1, a1 = m(X)
    assert not l0.requires_grad
    for l, a in ((l0, a0), (l1, a1)):
        assert torch.equal(l, logits)
        assert set(a) == set(aux) and "reconstruction" in a
        for k in aux:
            assert torch.equal(a[k], aux[k]), k
    assert torch.equal(predict(m, X), logits)
    assert m._rt.carry is None and not m.training and m.step == 0


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["micro", "mini", "micro_vit", "micro_fa"])
def test_stand_alone_blocks_under_no_grad(name, precision):
    m, cfg = build(name, precision)
    g = torch.Generator().manual_seed(5)
    h = torch.randn(3, m.n_tokens, cfg.n_embd, generator=g).to(DEV)
    h2 = torch.randn(3, m.n_tokens, cfg.n_embd, generator=g).to(DEV)
    if cfg.use_nvit:
        h, h2 = h / h.norm(dim=-1, keepdim=True), h2 / h2.norm(dim=-1, keepdim=True)
    blk, ca = m.transformer.h[0], m.cross_attention
    want_b, want_c = blk(h), ca(h, h2)
    assert want_b.requires_grad and want_c.requires_grad
    with torch.no_grad():
        got_b, got_c = blk(h), ca(h, h2)
    assert torch.equal(got_b, want_b) and torch.equal(got_c, want_c)


def _swiglu_launches(m, X, no_grad):
    from nvit_amd import ops
    torch.cuda.synchronize()
    ops.prof_enable(True)
    ops.prof_collect()
    try:
        if no_grad:
            with torch.no_grad():
                m(X)
        else:
            m(X)
        torch.cuda.synchronize()
    finally:
        ops.prof_enable(False)
    prof = ops.prof_collect()
    return prof["gemm_swiglu"]["launches"], prof["gemm_swiglu_act"]["launches"]


@pytest.mark.parametrize("name,extra", [("mini", 1), ("mini_k", 3)])
def test_no_grad_forward_takes_the_gate_only_gemm(name, extra):
    """FAILS WITHOUT THE FEATURE.  One fused SwiGLU GEMM per block (c_fc) and per cross-attention call (proj): one
    call without the Kohonen head, three with it.  B = 336 makes the smaller of the two, proj (M x 2C = 16 464 x 256),
    large enough for the fused kernel (ops.FUSE_MIN_ELEMS)."""
    from nvit_amd import ops
    m, cfg = build(name, "bf16")
    B = 336
    assert B * m.n_tokens * 2 * cfg.n_embd >= ops.FUSE_MIN_ELEMS
    X, _ = batch(cfg, B)
    m(X)   # warm-up: shadow tables, LDS attributes
    n = cfg.n_layer + extra
    assert _swiglu_launches(m, X, no_grad=True) == (0, n)
    assert _swiglu_launches(m, X, no_grad=False) == (n, 0)


def test_no_grad_forward_peak_memory_drops_by_a_uv_tensor():
    """FAILS WITHOUT THE FEATURE.  base at B = 8: M = 8 * 784 token rows, C = 768; the raw pre-activations uv of one
    block are [M, 8C] bf16 = M * 8C * 2 bytes = 77 070 336.  The old route is still reachable: with grad mode ON and no
    parameter requiring a gradient, autograd runs every block function's forward and drops what it saved at once -
    the launches and allocations of a no_grad call before this route existed.  Both peaks are
    max_memory_allocated() minus memory_allocated() before the call; the forward-only one must be lower by at least
    one uv (it is lower by more: the head tensors q, k, v are released before the MLP's tensors are allocated)."""
    m, cfg = build("base", "bf16")
    B = 8
    X, _ = batch(cfg, B)
    uv_bytes = B * m.n_tokens * 8 * cfg.n_embd * 2
    assert uv_bytes == 77070336
    for p in m.parameters():
        p.requires_grad_(False)

    def peak(no_grad):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        if no_grad:
            with torch.no_grad():
                out = m(X)
        else:
            out = m(X)
            assert not out[0].requires_grad
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, out[0]

    peak(True)   # warm-up: shadows and workspaces are allocated once and stay
    lean, l_lean = peak(True)
    old, l_old = peak(False)
    print(f"peak over the forward: forward-only {lean} B, old route {old} B, drop {old - lean} B = {(old - lean) / uv_bytes:.2f} uv")
    assert torch.equal(l_lean, l_old)
    assert lean + uv_bytes <= old


# ---------------------------------------------------------------------------------------------------------------
def _reference_loop(m, cfg, batches, eval_iters=None):
    """Trainer.validate and estimate_loss re-enacted with torch ops on the model's own logits (host side, double)."""
    tot = {"loss": 0.0, "t1": 0.0, "t5": 0.0}
    t1_f32 = torch.zeros((), dtype=torch.float32)
    t5_f32 = torch.zeros((), dtype=torch.float32)
    aux_tot, est, n = {}, [], 0
    for X, y in batches:
        with torch.no_grad():
            logits, aux = m(X)
        logits, yc = logits.cpu(), y.cpu()
        ce = F_.cross_entropy(logits, yc).item()
        maxk = min(5, logits.size(1))
        _, pred = logits.topk(maxk, 1, True, True)
        pred = pred.t()
        correct = pred.eq(yc.view(1, -1).expand_as(pred))
        c1, c5 = correct[0].float().sum().item(), correct[:maxk].float().sum().item()
        bs = yc.size(0)
        tot["loss"] += ce
        tot["t1"] += c1 * 100.0 / bs
        tot["t5"] += c5 * 100.0 / bs
        t1_f32 = t1_f32 + torch.tensor(c1, dtype=torch.float32) * 100.0 / bs
        t5_f32 = t5_f32 + torch.tensor(c5, dtype=torch.float32) * 100.0 / bs
        for k, v in aux.items():
            aux_tot[k] = aux_tot.get(k, 0.0) + v.item()
        loss = ce
        if cfg.use_kohonen:
            loss += 0.1 * aux["kohonen_consistency"].item() + 0.1 * aux["kohonen_smoothness"].item()
            loss += cfg.reconstruction_weight * aux["reconstruction"].item()
            loss += cfg.local_quantization_weight * aux["local_quantization"].item()
            loss += cfg.global_quantization_weight * aux["global_quantization"].item()
        est.append(loss)
        n += 1
    out = {"val/loss": tot["loss"] / n, "val/top1_accuracy": tot["t1"] / n, "val/top5_accuracy": tot["t5"] / n}
    f32 = {"val/top1_accuracy": t1_f32.item() / n, "val/top5_accuracy": t5_f32.item() / n}
    return out, f32, {k: v / n for k, v in aux_tot.items()}, est


class _Wrapped:   # what evaluate sees of the data-parallel wrapper: the bare model under .module
    def __init__(self, module):
        self.module = module


@pytest.mark.parametrize("train_flag", [True, False])
@pytest.mark.parametrize("name", ["micro", "micro_k"])
def test_validate_and_estimate_loss_match_the_reference_loop(name, train_flag):
    from nvit_amd import estimate_loss, validate
    m, cfg = build(name, "bf16", train=train_flag)
    batches = [batch(cfg, b, seed=100 + i) for i, b in enumerate((8, 8, 8, 3))]
    m.eval()
    ref, ref_f32, ref_aux, est = _reference_loop(m, cfg, batches)
    m.train(train_flag)
    nodes = ([m.local_kohonen.nodes.detach().clone(), m.global_kohonen.nodes.detach().clone()]
             if cfg.use_kohonen else [])
    step = m.step
    got = validate(m, iter(batches))
    print(name, "validate:", got, "reference:", ref)
    assert m.training == train_flag and m.step == step and m._rt.carry is None
    if cfg.use_kohonen:
        assert torch.equal(m.local_kohonen.nodes, nodes[0]) and torch.equal(m.global_kohonen.nodes, nodes[1])
    kk = {"val/consistency_loss": "kohonen_consistency", "val/smoothness_loss": "kohonen_smoothness",
          "val/local_quantization_loss": "local_quantization", "val/global_quantization_loss": "global_quantization"}
    assert set(got) == set(ref) | (set(kk) if cfg.use_kohonen else set())
    assert abs(got["val/loss"] - ref["val/loss"]) <= 2e-6 * max(1.0, abs(ref["val/loss"]))
    for k in ("val/top1_accuracy", "val/top5_accuracy"):
        # exact: the reference's per-batch formula count * 100 / batch size, summed in batch order in the device
        # accumulator's fp32, gives these bits; against the same sum in double only fp32's rounding remains
        assert got[k] == ref_f32[k], (k, got[k], ref_f32[k])
        assert abs(got[k] - ref[k]) <= 1e-5 * max(1.0, abs(ref[k]))
    for k, a in kk.items():
        if cfg.use_kohonen:
            assert abs(got[k] - ref_aux[a]) <= 2e-6 * max(1.0, abs(ref_aux[a])), k
    assert validate(_Wrapped(m), batches) == got
    for iters in (3, 10):
        want = sum(est[:iters]) / len(est[:iters])
        e = estimate_loss(m, iter(batches), iters)
        print(name, "estimate_loss", iters, e, want)
        assert abs(e - want) <= 2e-6 * max(1.0, abs(want))
    assert m.training == train_flag and m.step == step


@pytest.mark.parametrize("name", ["micro", "micro_k"])
def test_train_step_after_validate_is_the_train_step_without_it(name):
    """No stale carry, no changed cache, no moved SOM node or step counter: the optimizer step that follows a
    validate call is, bit for bit, the one taken without it."""
    from nvit_amd import validate
    from nvit_amd.train import train_step
    outs = []
    for with_validate in (False, True):
        m, cfg = build(name, "bf16", train=True)
        opt = m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
        X, y = batch(cfg, 8)
        train_step(m, opt, X, y, 1.0)
        if with_validate:
            validate(m, [batch(cfg, b, seed=50 + b) for b in (8, 5)])
        logits, loss, aux, gnorm = train_step(m, opt, X, y, 1.0)
        outs.append((logits, loss, gnorm, [p.detach().clone() for p in m.parameters()],
                     [b.detach().clone() for b in m.buffers()], m.step))
    a, b = outs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[5] == b[5]
    assert all(torch.equal(p, q) for p, q in zip(a[3], b[3]))
    assert all(torch.equal(p, q) for p, q in zip(a[4], b[4]))
