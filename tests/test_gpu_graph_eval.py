"""GPU: GraphedEval (predict / validate / estimate_loss with the forward replayed as a hipGraph) against the module-level
functions of nvit_amd.evaluate.  The captured graphs keep the eager fp32 additions in their order, so every comparison
is bitwise; the last batch of each loader is short and therefore takes the eager route inside the same call."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 8


def build(name, precision):
    from nvit_amd.config import named_config
    from nvit_amd.model import ViT
    from nvit_amd.train import normalize_matrices
    from nvit_amd.weights import load_formula_weights
    cfg = named_config(name)
    m = ViT(cfg)
    load_formula_weights(m, cfg)
    m = m.to(DEV).set_precision(precision).train()
    normalize_matrices(m)
    return m, cfg


def batch(cfg, n, seed):
    from nvit_amd.weights import synthetic_batch
    X, y = synthetic_batch(cfg, n, seed=seed)
    return X.to(DEV), y.to(DEV)


def _nodes(m):
    return [km.nodes.detach().clone() for km in (getattr(m, "local_kohonen", None), getattr(m, "global_kohonen", None))
            if km is not None]


def _check_against_eager(ge, m, batches, what):
    from nvit_amd import evaluate
    X = batches[0][0]
    got = ge.predict(X)
    want = evaluate.predict(m, X)
    assert torch.equal(got, want), (what, (got - want).abs().max().item())
    ge.predict(batches[1][0])
    assert torch.equal(got, want), (what, "predict returned a tensor that the next call overwrote")
    short = ge.predict(batches[2][0])   # another shape: eager
    assert short.shape[0] == 5 and torch.equal(short, evaluate.predict(m, batches[2][0])), what
    v_got, v_want = ge.validate(batches), evaluate.validate(m, batches)
    print(f"[{what}] validate {v_got}")
    assert v_got == v_want, (what, v_got, v_want)
    assert ge.validate(iter(batches)) == v_want, (what, "second call: the accumulator was not zeroed")
    e_got, e_want = ge.estimate_loss(batches, 2), evaluate.estimate_loss(m, batches, 2)
    print(f"[{what}] estimate_loss {e_got!r}")
    assert e_got == e_want, (what, e_got, e_want)
    # all three batches, the short one last (eager), and a loader that ends before eval_iters
    assert ge.estimate_loss(batches, 3) == evaluate.estimate_loss(m, batches, 3), what
    assert ge.estimate_loss(batches[:1], 4) == evaluate.estimate_loss(m, batches[:1], 4), what


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["micro", "micro_k", "micro_fa", "mini_vit"])
def test_graphed_eval_equals_eager_and_follows_the_weights(name, precision):
    from nvit_amd import GraphedEval
    from nvit_amd.train import train_step
    m, cfg = build(name, precision)
    batches = [batch(cfg, B, 11), batch(cfg, B, 12), batch(cfg, 5, 13)]
    opt = m.configure_optimizers(0.1, 1e-3, (0.9, 0.95), "cuda")
    train_step(m, opt, *batches[0])
    step, nodes = m.step, _nodes(m)
    assert m.training and step == 1
    ge = GraphedEval(m, *batches[0])
    _check_against_eager(ge, m, batches, f"{name} {precision}")
    assert m.training and m.step == step
    for a, b in zip(_nodes(m), nodes):
        assert torch.equal(a, b)
    m.eval()
    ge.predict(batches[0][0])
    assert not m.training
    m.train()
    # training goes on between evaluations: the same object must see the new weights
    before = ge.predict(batches[0][0])
    train_step(m, opt, *batches[1])
    nodes = _nodes(m)
    assert not torch.equal(ge.predict(batches[0][0]), before)
    _check_against_eager(ge, m, batches, f"{name} {precision} after a train step")
    assert m.training and m.step == step + 1
    for a, b in zip(_nodes(m), nodes):
        assert torch.equal(a, b)


def test_graphed_eval_uses_the_weights_given_to_it():
    from nvit_amd import GraphedEval, evaluate
    m, cfg = build("micro_k", "bf16")
    batches = [batch(cfg, B, 11), batch(cfg, B, 12)]
    ge = GraphedEval(m, *batches[0], consistency_weight=0.3, smoothness_weight=0.7)
    want = evaluate.estimate_loss(m, batches, 2, 0.3, 0.7)
    assert ge.estimate_loss(batches, 2) == want != evaluate.estimate_loss(m, batches, 2)
    with pytest.raises(ValueError):
        ge.estimate_loss(batches, 0)
    with pytest.raises(ValueError):
        ge.validate([])
