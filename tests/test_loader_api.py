"""CPU: the device-resident dataset (nvit_amd/data.py) up to the calls that need the device.  The numpy twin of the draw
(tests/loader_ref.py) is a bijection per (seed, epoch) and schedules positions as DESIGN.md §7 defines them; the loader
batch follows the batch-object protocol, is refused where it may not stand, saves and restores its state and gets its
checkpoint key; `eval_batches` cuts the dataset into contiguous slices with the short tail."""
import numpy as np
import pytest
import torch

import loader_ref as R
from nvit_amd import DeviceDataset
from nvit_amd.augment import AutoAugment
from nvit_amd.crop import RandomErasing, RandomResizedCrop, ResizeCenterCrop
from nvit_amd.data import DeviceLoader, LoaderBatch
from nvit_amd.mix import Mixup
from nvit_amd.randaug import RandAugment
from nvit_amd.stages import StagedBatch, chain

RRC, AA, RA, ERASE, MIX, RCC = RandomResizedCrop(32), AutoAugment("cifar10"), RandAugment(), RandomErasing(), Mixup(), ResizeCenterCrop(32)


def dataset(N=37, H=40, W=40, C=3, seed=0):
    g = np.random.default_rng(seed)
    return DeviceDataset(torch.from_numpy(g.integers(0, 256, (N, H, W, C), dtype=np.uint8)),
                         torch.from_numpy(g.integers(0, 10, (N,))))


# ------------------------------------------------------------------------------------------------ the twin's perm
@pytest.mark.parametrize("N", [1, 2, 3, 5, 16, 17, 1000, 4097, 50000])
def test_perm_is_a_bijection_that_differs_between_epochs_and_seeds(N):
    assert R.width(N) % 2 == 0 and R.width(N) >= 2 and (N - 1) < 2 ** R.width(N) and (N <= 4 or (N - 1) >= 2 ** (R.width(N) - 2))
    x = np.arange(N)
    seen = {}
    for seed, epoch in ((0, 0), (0, 1), (7, 0), (2 ** 63 + 11, 2 ** 32 + 5), (0, 2 ** 32)):
        p, walk = R.perm(x, N, seed, epoch, return_walk=True)
        assert p.dtype == np.int64 and np.array_equal(np.sort(p), x), (seed, epoch)
        assert walk.min() >= 1 and walk.mean() <= 4.0 and walk.max() <= 64, (seed, epoch, walk.mean(), walk.max())
        seen[(seed, epoch)] = p
    if N >= 1000:   # (a permutation of a handful of values may well repeat)
        keys = list(seen)
        for i, a in enumerate(keys):
            for b in keys[:i]:
                assert (seen[a] == seen[b]).mean() < 0.02, (a, b)
    # evaluated per element: any subset in any order gives the same values
    some = np.array([N - 1, 0, N // 2, N - 1])
    assert np.array_equal(R.perm(some, N, 7, 0), seen[(7, 0)][some])


def test_width_is_the_smallest_even_number_of_bits_that_holds_n_minus_one():
    assert [R.width(N) for N in (1, 2, 3, 4, 5, 16, 17, 64, 65, 256, 257, 50000, 1281167)] == \
        [2, 2, 2, 2, 4, 4, 6, 6, 8, 8, 10, 16, 22]


# ------------------------------------------------------------------------------------------------ the schedule
def test_drop_last_leaves_images_out_and_every_other_appears_once_per_epoch():
    N, B = 37, 8
    assert R.steps_per_epoch(N, B) == 4 and N - 4 * B == 5
    for epoch in (0, 1, 5):
        idx = np.concatenate([R.draw(3, epoch * 4 + t, N, B) for t in range(4)])
        assert len(set(idx.tolist())) == 32 and idx.min() >= 0 and idx.max() < N
        assert sorted(idx.tolist()) == sorted(R.perm(np.arange(32), N, 3, epoch).tolist())
    e0, e1 = (set(np.concatenate([R.draw(3, e * 4 + t, N, B) for t in range(4)]).tolist()) for e in (0, 1))
    assert e0 != e1   # other images are left out in another epoch


def test_two_ranks_see_the_one_rank_global_batch_row_for_row():
    N = 37
    assert R.steps_per_epoch(N, 4, 2) == R.steps_per_epoch(N, 8) == 4
    for step in range(9):   # two epoch borders: steps 3|4 and 7|8
        whole = R.draw(5, step, N, 8)
        parts = np.concatenate([R.draw(5, step, N, 4, world_size=2, rank=r) for r in (0, 1)])
        assert np.array_equal(whole, parts), step
        assert R.schedule(step, N, 8)[:2] == divmod(step, 4) == R.schedule(step, N, 4, 2, 1)[:2]


def test_repeats_show_every_used_image_exactly_that_often():
    N, B, rep = 37, 8, 3
    S = R.steps_per_epoch(N, B, repeats=rep)
    assert S == 13                      # 111 // 8
    for epoch in (0, 1):
        idx = np.concatenate([R.draw(1, epoch * S + t, N, B, repeats=rep) for t in range(S)])
        used, counts = np.unique(idx, return_counts=True)
        whole = (S * B) // rep         # images [0, whole) of the permutation appear `rep` times, one more is cut short
        assert (counts[np.isin(used, R.perm(np.arange(whole), N, 1, epoch))] == rep).all() and counts.max() == rep
        assert len(used) == whole + (1 if (S * B) % rep else 0)
        # the copies of an image sit next to each other
        assert np.array_equal(idx, R.perm(np.arange(S * B) // rep, N, 1, epoch))


def test_without_shuffle_the_position_is_the_image():
    for step in (0, 3, 4, 9):
        assert np.array_equal(R.draw(9, step, 37, 8, repeats=3, shuffle=False), ((step % 13) * 8 + np.arange(8)) // 3)
        assert np.array_equal(R.draw(9, step, 37, 4, 2, 1, shuffle=False), (step % 4) * 8 + 4 + np.arange(4))


# ------------------------------------------------------------------------------------------------ API
def test_dataset_and_loader_check_their_arguments():
    u8, y = torch.zeros(6, 8, 8, 3, dtype=torch.uint8), torch.zeros(6, dtype=torch.int64)
    for bad, exc in (((u8.float(), y), TypeError), ((u8, y.int()), TypeError), ((u8.numpy(), y), TypeError),
                     ((u8[0], y), ValueError), ((u8[..., :2], y), ValueError), ((u8, y[:5]), ValueError),
                     ((u8, y[:, None]), ValueError), ((u8[:, :, ::2], y), ValueError), ((u8[:0], y[:0]), ValueError)):
        with pytest.raises(exc):
            DeviceDataset(*bad)
    ds = DeviceDataset(u8, y)
    assert len(ds) == ds.N == 6 and ds.device == u8.device and ds.images is u8 and ds.labels is y and ds.to("cpu") is ds
    for kw, exc in ((dict(batch_size=0), ValueError), (dict(batch_size=2.0), TypeError), (dict(batch_size=True), TypeError),
                    (dict(batch_size=7), ValueError),                      # S == 0
                    (dict(batch_size=4, world_size=2), ValueError),        # S == 0 for the global batch
                    (dict(batch_size=2, world_size=0), ValueError), (dict(batch_size=2, world_size=2, rank=2), ValueError),
                    (dict(batch_size=2, rank=-1), ValueError), (dict(batch_size=2, repeats=0), ValueError),
                    (dict(batch_size=2, shuffle=1), TypeError), (dict(batch_size=2, seed=-1), ValueError),
                    (dict(batch_size=2, seed="0"), TypeError)):
        with pytest.raises(exc):
            ds.loader(**kw)
    ld = ds.loader(4, world_size=1, repeats=3)   # 18 positions: the repeats make a global batch fit that N alone would not
    assert ds.loader(batch_size=7, repeats=2).steps_per_epoch == 1
    assert isinstance(ld, DeviceLoader) and ld.steps_per_epoch == 4 and ld.step == 0 and ld.epoch == 0 and ld.global_batch == 4
    assert ds.loader(2, world_size=3, rank=2).first_index == 4
    with pytest.raises(RuntimeError):
        ld.draw()                        # no CPU path
    with pytest.raises(RuntimeError):
        ld.to("cpu")
    with pytest.raises(RuntimeError):
        ds.take(torch.zeros(2, dtype=torch.int64))


def test_the_loader_batch_follows_the_protocol_in_every_legal_chain():
    ds = dataset()
    ld = ds.loader(8)
    xb = ld.batch()
    assert isinstance(xb, LoaderBatch) and isinstance(xb, StagedBatch) and xb.key == "data" and chain(xb) == [xb]
    assert tuple(xb.shape) == (8, 40, 40, 3) and xb.source() is ds.images and xb.inner is ds.images and xb.images is ds.images
    assert xb.loader is ld and xb.stage is ld and xb.fit_key() == (ld,) and xb.device == ds.images.device
    assert xb.rebind(ds.images).source() is ds.images and ld.batch(ds.images).loader is ld
    with pytest.raises(ValueError):
        xb.rebind(ds.images.clone())     # a loader batch stands on its dataset's own tensor
    same = dataset(H=32, W=32)
    for outer, shape in ((lambda b: AA.batch(b), (8, 32, 32, 3)), (lambda b: RA.batch(b), (8, 32, 32, 3)),
                         (lambda b: ERASE.batch(AA.batch(b)), (8, 3, 32, 32)), (lambda b: MIX.batch(RA.batch(b)), (8, 32, 32, 3))):   # (a Mixup reports the shape of what it wraps)
        X = outer(same.loader(8).batch())
        assert tuple(X.shape) == shape and X.source() is same.images and chain(X)[-1].key == "data"
    full = MIX.batch(ERASE.batch(RA.batch(RRC.batch(xb)), 0.4, 0.2))
    assert [b.key for b in chain(full)] == ["mix", "erase", "augment", "crop", "data"]
    assert tuple(full.shape) == (8, 3, 32, 32) and full.source() is ds.images and full.B == 8
    assert tuple(ERASE.batch(RRC.batch(xb)).shape) == (8, 3, 32, 32) and tuple(RRC.batch(xb).shape) == (8, 32, 32, 3)
    again = full.rebind(ds.images)
    assert [b.stage for b in chain(again)] == [b.stage for b in chain(full)] and chain(again)[1].fit_key() == (ERASE, 0.4, 0.2)
    from nvit_amd.train import _unwrap_input, _wrap_input
    stages, inner = _unwrap_input(full)
    assert list(stages) == ["mix", "erase", "augment", "crop", "data"] and stages["data"] is ld and inner is ds.images
    assert _unwrap_input(_wrap_input(stages, inner))[0] == stages
    # the Mixup's label check is satisfied from the dataset
    full.check_labels(None)
    assert full.labels().dtype == torch.int64 and full.labels().shape == (8,) and AA.batch(torch.zeros(2, 8, 8, 3, dtype=torch.uint8)).labels() is None
    with pytest.raises(TypeError):
        MIX.batch(torch.zeros(8, 3, 32, 32)).check_labels(None)   # no loader inside: y is needed as before


def test_illegal_nestings_with_a_loader_batch_are_type_errors():
    ds = dataset()
    xb = ds.loader(8).batch()
    f32 = torch.zeros(8, 3, 32, 32)
    for name, bad in {"erase(data)": lambda: ERASE.batch(xb), "mix(data)": lambda: MIX.batch(xb), "rcc(data)": lambda: RCC.batch(xb),
                      "mix(rrc(data))": lambda: MIX.batch(RRC.batch(xb)), "rrc(rrc(data))": lambda: RRC.batch(RRC.batch(xb)),
                      "aa(aa(data))": lambda: AA.batch(AA.batch(xb)), "rrc(aa(data))": lambda: RRC.batch(AA.batch(xb)),
                      "resolve(data)": lambda: xb.resolve(None), "resolve(rrc(data))": lambda: RRC.batch(xb).resolve(None)}.items():
        with pytest.raises(TypeError):
            bad()
        assert name
    with pytest.raises(ValueError):
        AA.batch(dataset(H=32, W=30).loader(8).batch())   # W % 4, as for a tensor


def test_a_step_refuses_a_loader_batch_alone_and_a_y_beside_it():
    from nvit_amd.config import named_config
    from nvit_amd.evaluate import GraphedEval, _model_input, predict
    from nvit_amd.model import ViT
    from nvit_amd.train import GraphedTrainStep, _check_step_args, _unwrap_input, train_step
    ds = dataset(H=32, W=32)
    ld = ds.loader(8)
    model = ViT(named_config("micro"))
    y = torch.zeros(8, dtype=torch.int64)
    for X in (ld.batch(), RRC.batch(dataset().loader(8).batch())):   # uint8: no model input
        with pytest.raises(TypeError):
            train_step(model, None, X, None)
        with pytest.raises(TypeError):
            _unwrap_input(X)
    for X in (AA.batch(ld.batch()), MIX.batch(ERASE.batch(RA.batch(ld.batch())))):
        with pytest.raises(ValueError, match="y=None"):
            train_step(model, None, X, y)
        with pytest.raises(ValueError, match="y=None"):
            GraphedTrainStep(model, None, X, y)
        with pytest.raises(ValueError, match="y=None"):
            X.resolve(y)
        _check_step_args(None, X, 2, False, None)
        with pytest.raises(ValueError):
            _check_step_args(None, X, 3, False, None)   # accumulation divides the loader's batch size
        # evaluation takes eval_batches, not the training stage
        for call in (lambda: predict(model, X), lambda: GraphedEval(model, X, y), lambda: _model_input(X)):
            with pytest.raises(TypeError, match="eval_batches"):
                call()
    with pytest.raises(TypeError):
        predict(model, ld.batch())
    assert ld.step == 0


def test_state_dict_round_trip_and_refused_mismatch():
    ds = dataset()
    a = ds.loader(4, seed=5, world_size=2, rank=1, repeats=3)
    assert a.state_dict() == {"seed": 5, "step": 0, "N": 37, "batch_size": 4, "world_size": 2, "rank": 1, "repeats": 3,
                              "shuffle": True}
    state = {**a.state_dict(), "step": 11, "seed": 9}
    b = ds.loader(4, seed=0, world_size=2, rank=1, repeats=3)
    b.load_state_dict(state)
    assert b.state_dict() == state and b.step == 11 and b.epoch == 11 // b.steps_per_epoch and b.seed == 9
    for key, other in (("N", 38), ("batch_size", 8), ("world_size", 1), ("rank", 0), ("repeats", 1), ("shuffle", False),
                       ("shuffle", 1)):
        with pytest.raises(ValueError, match=key):
            b.load_state_dict({**state, key: other})
    with pytest.raises(ValueError):
        b.load_state_dict({k: v for k, v in state.items() if k != "repeats"})
    with pytest.raises(ValueError):
        b.load_state_dict({**state, "step": -1})
    assert b.state_dict() == state       # a refused state changes nothing


def test_the_checkpoint_gains_the_key_only_with_a_loader(tmp_path):
    from nvit_amd.checkpoint import build_checkpoint, save_checkpoint
    from nvit_amd.config import named_config
    from nvit_amd.model import ViT
    model = ViT(named_config("micro"))
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    ld = dataset().loader(8, seed=3)
    ld.load_state_dict({**ld.state_dict(), "step": 6})
    plain = build_checkpoint(model, opt, 1, {})
    with_ld = build_checkpoint(model, opt, 1, {}, loader=ld)
    assert "loader" not in plain and set(with_ld) == set(plain) | {"loader"} and with_ld["loader"] == ld.state_dict()
    path = save_checkpoint(tmp_path / "ck.pt", model, opt, 1, {}, loader=ld)
    from nvit_amd.checkpoint import _numpy_safe_globals
    with torch.serialization.safe_globals(_numpy_safe_globals()):      # (for rng_state_numpy, as load_checkpoint does)
        ck = torch.load(path, map_location="cpu", weights_only=True)   # plain values: the weights-only load takes the key
    fresh = dataset().loader(8)
    fresh.load_state_dict(ck["loader"])
    assert fresh.state_dict() == ld.state_dict() and fresh.step == 6 and fresh.epoch == 1


def test_eval_batches_are_contiguous_slices_with_the_short_tail():
    ds = dataset(N=11)
    got = list(ds.eval_batches(4, RCC))
    assert [tuple(X.shape) for X, _ in got] == [(4, 3, 32, 32), (4, 3, 32, 32), (3, 3, 32, 32)]
    for k, (X, y) in enumerate(got):
        assert X.crop is RCC and X.key is None and torch.equal(X.source(), ds.images[4 * k:4 * k + 4])
        assert X.source().data_ptr() == ds.images[4 * k:].data_ptr()       # a view, no copy
        assert torch.equal(y, ds.labels[4 * k:4 * k + 4])
    assert len(list(ds.eval_batches(11, RCC))) == 1 and len(list(ds.eval_batches(12, RCC))) == 1
    with pytest.raises(TypeError):
        ds.eval_batches(4, RRC)
    with pytest.raises(ValueError):
        ds.eval_batches(0)
    it = ds.eval_batches(4)              # without a transform the first batch already needs the device
    with pytest.raises(RuntimeError):
        next(it)
