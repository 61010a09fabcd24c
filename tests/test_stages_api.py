"""CPU: the batch-object protocol of nvit_amd.stages.  Every chain the input pipeline accepts reports its shape, device
and innermost tensor, is rebuilt by `rebind` from the same stage objects, and unwraps to the dict the captured step keeps;
every other nesting is refused with TypeError; and the affine arithmetic that AutoAugment's and RandAugment's tables share
writes the recorded rows (tests/golden/affine_rows.npz, tools/make_golden_affine_rows.py)."""
import itertools
import os

import numpy as np
import pytest
import torch

from nvit_amd import augment, randaug
from nvit_amd.augment import AugmentedBatch, AutoAugment
from nvit_amd.crop import (CenterCroppedBatch, CroppedBatch, ErasedBatch, RandomErasing, RandomResizedCrop,
                           ResizeCenterCrop)
from nvit_amd.mix import MixedBatch, Mixup
from nvit_amd.randaug import RandAugment
from nvit_amd.stages import StagedBatch, chain
from nvit_amd.train import _unwrap_input, _wrap_input

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "affine_rows.npz")
RRC, AA, RA, ERASE, MIX, RCC = RandomResizedCrop(32), AutoAugment("cifar10"), RandAugment(), RandomErasing(), Mixup(), ResizeCenterCrop(32)
MEAN, STD = 0.4, 0.2


def legal_chains():
    """(crop or None, augmentation or None, erase or None, mix or None) of every chain a step accepts: all but the empty
    one, the crop alone (uint8: no model input) and the crop directly under the Mixup (which takes fp32)."""
    for spec in itertools.product((None, RRC), (None, AA, RA), (None, ERASE), (None, MIX)):
        crop, aug, erase, mix = spec
        if any(spec) and not (crop and not aug and not erase):
            yield spec


def build(spec, src=None):
    crop, aug, erase, mix = spec
    if src is None:
        src = (torch.zeros(4, 40, 40, 3, dtype=torch.uint8) if crop else torch.zeros(4, 32, 32, 3, dtype=torch.uint8) if aug
               else torch.zeros(4, 3, 32, 32))
    X = src
    if crop:
        X = crop.batch(X)
    if aug:
        X = aug.batch(X)
    if erase:
        X = erase.batch(X, MEAN, STD)
    if mix:
        X = mix.batch(X)
    return X, src


def test_there_are_21_legal_chains_and_they_cover_the_pinned_ones():
    specs = list(legal_chains())
    assert len(specs) == 21
    for pinned in ((RRC, AA, ERASE, MIX), (RRC, AA, None, None), (RRC, None, ERASE, None), (None, AA, ERASE, None),
                   (None, None, ERASE, None), (None, None, ERASE, MIX), (RRC, None, ERASE, MIX), (RRC, AA, None, MIX),
                   (None, None, None, MIX), (RRC, RA, ERASE, MIX)):   # those of test_crop_api.py and test_randaug_api.py
        assert pinned in specs


@pytest.mark.parametrize("spec", list(legal_chains()), ids=lambda s: "-".join(type(o).__name__ for o in s if o))
def test_every_legal_chain_follows_the_protocol(spec):
    crop, aug, erase, mix = spec
    X, src = build(spec)
    classes = [c for c, o in ((MixedBatch, mix), (ErasedBatch, erase), (AugmentedBatch, aug), (CroppedBatch, crop)) if o]
    objects = [o for o in (mix, erase, aug, crop) if o]
    assert isinstance(X, StagedBatch) and [type(b) for b in chain(X)] == classes
    assert [b.stage for b in chain(X)] == objects and [b.key for b in chain(X)] == [c.key for c in classes]
    # the outermost shape: fp32 [B,C,H,W] behind an erasing, else what the augmentation sees, else the tensor's
    assert tuple(X.shape) == ((4, 3, 32, 32) if erase or not aug else (4, 32, 32, 3)) and X.shape[0] == 4
    assert X.device == src.device and X.source() is src
    # the named views of the two generic attributes
    for b in chain(X):
        assert getattr(b, b.key) is b.stage and (b.u8 if b.key in ("crop", "augment") else b.X) is b.inner
    if erase:
        e = chain(X)[1 if mix else 0]
        assert (e.mean, e.std) == (MEAN, STD) and e.fit_key() == (erase, MEAN, STD)
    if mix:
        assert X.B == 4
    # rebind: the same classes around the same stage objects, mean and std carried, another innermost tensor
    other = torch.ones_like(src)
    Y = X.rebind(other)
    assert Y is not X and Y.source() is other and X.source() is src
    assert [type(b) for b in chain(Y)] == classes and [b.stage for b in chain(Y)] == objects
    assert [b.fit_key() for b in chain(Y)] == [b.fit_key() for b in chain(X)] and tuple(Y.shape) == tuple(X.shape)
    # the dict view a captured step is built from
    want = {k: v for k, v in (("mix", mix), ("erase", (erase, MEAN, STD) if erase else None), ("augment", aug),
                              ("crop", crop)) if v}
    stages, inner = _unwrap_input(X)
    assert stages == want and list(stages) == list(want) and inner is src
    Z = _wrap_input(stages, other)
    assert [type(b) for b in chain(Z)] == classes and _unwrap_input(Z) == (want, other)


def test_a_tensor_and_the_evaluation_batch_are_no_chain():
    f32, u8 = torch.zeros(4, 3, 32, 32), torch.zeros(4, 40, 40, 3, dtype=torch.uint8)
    assert chain(f32) == [] and _unwrap_input(f32) == ({}, f32)
    xb = RCC.batch(u8)
    assert isinstance(xb, CenterCroppedBatch) and isinstance(xb, StagedBatch) and xb.key is None and chain(xb) == []
    assert tuple(xb.shape) == (4, 3, 32, 32) and xb.device == u8.device and xb.source() is u8 and xb.crop is RCC and xb.u8 is u8
    assert xb.fit_key() == RCC.params() == ResizeCenterCrop(32).batch(u8).fit_key() != ResizeCenterCrop(32, 0.9).batch(u8).fit_key()
    other = torch.ones_like(u8)
    yb = xb.rebind(other)
    assert type(yb) is CenterCroppedBatch and yb.crop is RCC and yb.source() is other


def illegal_nestings():
    u8, u32, f32 = (torch.zeros(4, 40, 40, 3, dtype=torch.uint8), torch.zeros(4, 32, 32, 3, dtype=torch.uint8),
                    torch.zeros(4, 3, 32, 32))
    bad = {"rrc(erase)": lambda: RRC.batch(ERASE.batch(f32)), "rrc(mix)": lambda: RRC.batch(MIX.batch(f32)),
           "rrc(rrc)": lambda: RRC.batch(RRC.batch(u8)), "erase(mix)": lambda: ERASE.batch(MIX.batch(f32)),
           "erase(erase)": lambda: ERASE.batch(ERASE.batch(f32)), "mix(rrc)": lambda: MIX.batch(RRC.batch(u8)),
           "mix(mix)": lambda: MIX.batch(MIX.batch(f32)), "unwrap(rrc)": lambda: _unwrap_input(RRC.batch(u8)),
           "resolve(rrc)": lambda: RRC.batch(u8).resolve(None),
           # evaluation's batch object inside a training stage, and the training batch objects inside evaluation's
           "rrc(rcc)": lambda: RRC.batch(RCC.batch(u8)), "erase(rcc)": lambda: ERASE.batch(RCC.batch(u8)),
           "mix(rcc)": lambda: MIX.batch(RCC.batch(u8)), "rcc(rrc)": lambda: RCC.batch(RRC.batch(u8)),
           "rcc(erase)": lambda: RCC.batch(ERASE.batch(f32)), "rcc(mix)": lambda: RCC.batch(MIX.batch(f32)),
           "rcc(rcc)": lambda: RCC.batch(RCC.batch(u8))}
    for name, aug in (("aa", AA), ("ra", RA)):
        bad.update({f"rrc({name})": lambda aug=aug: RRC.batch(aug.batch(u32)), f"{name}(erase)": lambda aug=aug: aug.batch(ERASE.batch(f32)),
                    f"{name}(mix)": lambda aug=aug: aug.batch(MIX.batch(f32)), f"{name}({name})": lambda aug=aug: aug.batch(aug.batch(u32)),
                    f"{name}(rcc)": lambda aug=aug: aug.batch(RCC.batch(u8)), f"rcc({name})": lambda aug=aug: RCC.batch(aug.batch(u32))})
    return bad


@pytest.mark.parametrize("name", sorted(illegal_nestings()))
def test_every_other_nesting_is_a_type_error(name):
    with pytest.raises(TypeError):
        illegal_nestings()[name]()


def test_the_shared_affine_helper_writes_the_recorded_rows():
    g = np.load(GOLDEN)
    cases = [tuple(int(v) for v in c) for c in g["cases"]]
    geometric = [augment.OPS.index(n) for n in ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate")]
    assert sorted(cases) == sorted((o, m, sg, H, W) for o in geometric for m in (0, 5, 9) for sg in (0, 1)
                                   for H, W in ((32, 32), (24, 40), (1, 1)))
    assert g["augment"].shape == (len(cases), augment.ROW) and g["randaug"].shape == (len(cases), randaug.ROW)
    for i, (op, m, sign, H, W) in enumerate(cases):
        name = augment.OPS[op]
        assert augment.op_row(name, augment.magnitude(name, m, sign, W), H, W) == g["augment"][i].tolist(), (name, m, sign, H, W)
        value = randaug.level_arg(name, float(m), sign, True, H, W)
        assert randaug.op_row(name, value, "bilinear", H=H, W=W) == g["randaug"][i].tolist(), (name, m, sign, H, W)
    # both tables hold the one function's coefficients: RandAugment's as fp64, AutoAugment's rounded to 16.16
    a = augment.affine_coefficients("Rotate", 30.0, 24, 40)
    assert randaug.op_row("Rotate", 30.0, H=24, W=40)[2:14] == [v for c in a for v in randaug._f64_ints(c)]
    assert augment.op_row("Rotate", 30.0, 24, 40)[1:3] == [augment._fix(a[0]), augment._fix(a[1])]
