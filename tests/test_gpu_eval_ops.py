"""GPU: the two kernels of the forward-only route, op by op.

nvit_gemm_nt_swiglu_act (the gate-only epilogue of the persistent NT GEMM) must write the bits nvit_gemm_nt_swiglu
writes into xm, and nothing outside [M, F]; nvit_eval_metrics must reproduce F.cross_entropy + topk of the reference's
Trainer.compute_accuracy / validate (train.py:563-575, 595-613) from one launch."""
import pytest
import torch
import torch.nn.functional as F_

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def ops_():
    from nvit_amd import ops
    return ops


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@pytest.fixture
def sched():
    """sets the persistent GEMMs' tile schedule; static (the single-process default) is put back afterwards"""
    from nvit_amd import _lib
    lib = _lib.load()
    yield lambda dynamic: lib.nvit_set_gemm_sched(int(dynamic))
    lib.nvit_set_gemm_sched(0)


# (M, F, K): the shape of the existing fused-SwiGLU test, a ragged M, and c_fc of the base model at 4 images
SWIGLU_SHAPES = [(6000, 512, 256), (5123, 512, 256), (4 * 784, 3072, 768)]


@pytest.mark.parametrize("dynamic", [False, True], ids=["static", "dynamic"])
@pytest.mark.parametrize("use_gs", [True, False], ids=["gs", "nogs"])
@pytest.mark.parametrize("M,F,K", SWIGLU_SHAPES)
def test_gemm_nt_swiglu_act_is_the_fused_gate_bit_for_bit(M, F, K, use_gs, dynamic, sched):
    ops = ops_()
    from nvit_amd._lib import BF16, check, load
    d_ = dev()
    A = rnd(M, K, seed=1).bfloat16().to(d_)
    W = (rnd(2 * F, K, seed=2) * 0.05).bfloat16().to(d_)
    gs = (rnd(2 * F, seed=3, scale=0.1) + 1).to(d_) if use_gs else None
    gscale = 3.0 if use_gs else 1.0
    assert ops.fusable(BF16, M, 2 * F, K)
    sched(dynamic)
    _, xm = ops.gemm_nt_swiglu(A, W, M, F, K, gs, gscale)
    xm_act = ops.gemm_nt_swiglu_act(A, W, M, F, K, gs, gscale)
    assert xm_act.shape == (M, F) and xm_act.dtype == torch.bfloat16
    assert torch.equal(xm_act, xm)
    # against the fp32 gate of the fp32 product, at the bound of test_fused_gemm_swiglu_and_qknorm_match_unfused
    z = A.float() @ W.float().t()
    if use_gs:
        z = z * (gs * gscale)
    zz = z.reshape(M, F // 16, 2, 16)
    want = (zz[:, :, 0] * (zz[:, :, 1] * torch.sigmoid(zz[:, :, 1]))).reshape(M, F)
    err = (xm_act.float() - want).abs().max().item()
    print(f"swiglu_act M={M} F={F} K={K} gs={use_gs} dyn={dynamic}: max err {err:.3e} (|want|max {want.abs().max().item():.3e})")
    assert err < 2e-2 * max(1.0, want.abs().max().item())
    # guard band: xm inside a larger buffer of a sentinel (0x7f7f as bf16 bits), rows above and below
    PAD = 64
    buf = torch.full(((M + 2 * PAD) * F,), 0x7F7F, dtype=torch.int16, device=d_)
    inner = buf[PAD * F:(PAD + M) * F]
    check(load().nvit_gemm_nt_swiglu_act(BF16, A.data_ptr(), K, W.data_ptr(), K, inner.data_ptr(), M, F, K,
                                         None if gs is None else gs.data_ptr(), gscale, None,
                                         torch.cuda.current_stream().cuda_stream), "nvit_gemm_nt_swiglu_act")
    torch.cuda.synchronize()
    assert torch.equal(inner.view(torch.bfloat16).reshape(M, F), xm)
    assert bool((buf[:PAD * F] == 0x7F7F).all()) and bool((buf[(PAD + M) * F:] == 0x7F7F).all())


def test_gemm_nt_swiglu_act_refuses_what_the_fused_kernel_does_not_take():
    ops = ops_()
    d_ = dev()
    A = rnd(512, 96, seed=1).bfloat16().to(d_)      # K % 64 != 0
    W = rnd(512, 96, seed=2).bfloat16().to(d_)
    with pytest.raises(RuntimeError):
        ops.gemm_nt_swiglu_act(A, W, 512, 256, 96, None, 1.0)


# ---------------------------------------------------------------------------------------------------------------
def ref_metrics(logits, y):
    """One batch as the reference computes it on the CPU (train.py:563-575, 595): (loss, #top1, #topk) - the
    counts are integers; the reference turns them into count * 100.0 / batch_size."""
    loss = F_.cross_entropy(logits, y).item()
    maxk = min(5, logits.size(1))
    _, pred = logits.topk(maxk, 1, True, True)
    pred = pred.t()
    correct = pred.eq(y.view(1, -1).expand_as(pred))
    return loss, int(correct[0].float().sum().item()), int(correct[:maxk].float().sum().item())


def tie_free_logits(B, N, seed):
    """Seeded rows without equal logits BY CONSTRUCTION (128 000 independent normal draws do collide in fp32): row b is
    a random permutation of the N distinct levels (j + u_b) * 12 / N - 6, u_b in [0, 1) per row; checked below."""
    g = torch.Generator().manual_seed(seed)
    perm = torch.stack([torch.randperm(N, generator=g) for _ in range(B)]).double()
    x = ((perm + torch.rand(B, 1, generator=g).double()) * (12.0 / N) - 6.0).float()
    s = x.sort(dim=1).values
    assert bool((s[:, 1:] != s[:, :-1]).all()), "a row has equal logits: topk's tie order would matter"
    # labels: every third row's largest logit, every third row's third largest, the rest random - hits, top-k-only
    # hits and misses all occur
    y = torch.randint(0, N, (B,), generator=g)
    order = x.argsort(dim=1, descending=True)
    y[0::3] = order[0::3, 0]
    y[1::3] = order[1::3, min(2, N - 1)]
    return x, y


def run_metrics(logits, y, acc=None):
    ops = ops_()
    if acc is None:
        acc = torch.zeros(4, device=dev(), dtype=torch.float32)
    ops.eval_metrics(logits.to(dev()), y.to(dev()), acc)
    return acc


def f32(x):
    return torch.tensor(x, dtype=torch.float32)


@pytest.mark.parametrize("B,N", [(1, 3), (7, 10), (33, 100), (128, 1000), (512, 100)])
def test_eval_metrics_match_cross_entropy_and_topk(B, N):
    """Loss at the bar of test_ce_loss_fwd_bwd; the accuracies exact: the count of correct rows recovered from the
    accumulator is the reference's integer, and the stored value is the reference's formula count * 100 / B evaluated
    in the accumulator's own fp32 (one exact product, one correctly rounded division), bit for bit."""
    logits, y = tie_free_logits(B, N, seed=100 + B)
    loss, c1, ck = ref_metrics(logits, y)
    acc = run_metrics(logits, y).cpu()
    print(f"eval_metrics B={B} N={N}: loss {acc[0].item():.7f} (ref {loss:.7f}) top1 {acc[1].item()} top{min(5, N)} {acc[2].item()}")
    assert abs(acc[0].item() - loss) <= 2e-6 * max(1.0, abs(loss))
    assert round(acc[1].item() * B / 100.0) == c1 and round(acc[2].item() * B / 100.0) == ck
    assert acc[1].item() == (f32(c1) * 100.0 / B).item() and acc[2].item() == (f32(ck) * 100.0 / B).item()
    assert abs(acc[1].item() - c1 * 100.0 / B) <= 1e-5 and abs(acc[2].item() - ck * 100.0 / B) <= 1e-5
    assert acc[3].item() == 1.0
    # reproducible run to run (fixed-order reduction)
    assert torch.equal(run_metrics(logits, y).cpu(), acc)


def test_eval_metrics_rank_five_counts_and_rank_six_does_not():
    N = 12
    base = torch.arange(N, dtype=torch.float32) * 0.5     # logit j = j / 2: class N-1 is the largest
    logits = torch.stack([base, base, base])
    y = torch.tensor([N - 5, N - 6, N - 1])               # ranked exactly 5th, exactly 6th, 1st
    loss, c1, ck = ref_metrics(logits, y)
    assert (c1, ck) == (1, 2)
    acc = run_metrics(logits, y).cpu()
    assert acc[1].item() == (f32(1) * 100.0 / 3).item() and acc[2].item() == (f32(2) * 100.0 / 3).item()
    assert abs(acc[0].item() - loss) <= 2e-6 * max(1.0, abs(loss))
    # equal logits: the lower index wins, so the target at the higher index of a tied pair is ranked one lower
    tied = torch.tensor([[1.0, 1.0, 0.0, -1.0]])
    assert run_metrics(tied, torch.tensor([0])).cpu()[1].item() == 100.0
    assert run_metrics(tied, torch.tensor([1])).cpu()[1].item() == 0.0
    # fewer than five classes: maxk = min(5, N), every row is a top-k hit
    l3, y3 = tie_free_logits(4, 3, seed=9)
    assert run_metrics(l3, y3).cpu()[2].item() == 100.0


def test_eval_metrics_accumulate_means_of_batch_means():
    """Two calls with different B add their per-batch means (what Trainer.validate sums, train.py:603-613); the
    mean over all rows is a different number, and the accumulator must not hold it."""
    N = 10
    la, ya = tie_free_logits(6, N, seed=21)
    lb, yb = tie_free_logits(2, N, seed=23)
    yb = lb.argmax(dim=1)                                   # the short batch is all correct
    (loss_a, a1, ak), (loss_b, b1, bk) = ref_metrics(la, ya), ref_metrics(lb, yb)
    acc = run_metrics(la, ya)
    acc = run_metrics(lb, yb, acc).cpu()
    assert acc[3].item() == 2.0
    assert abs(acc[0].item() - (loss_a + loss_b)) <= 2e-6 * max(1.0, abs(loss_a + loss_b))
    assert acc[1].item() == (f32(a1) * 100.0 / 6 + f32(b1) * 100.0 / 2).item()
    assert acc[2].item() == (f32(ak) * 100.0 / 6 + f32(bk) * 100.0 / 2).item()
    pooled = (a1 + b1) * 100.0 / 8
    assert abs(acc[1].item() / 2 - pooled) > 1.0, "the cases must tell the two rules apart"
