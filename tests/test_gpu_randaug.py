"""GPU: the on-device RandAugment (nvit_randaug_draw / nvit_randaug_apply, nvit_amd/randaug.py) against the numpy
restatement tests/randaug_ref.py, which tests/test_randaug_ref.py pins to Pillow.  The apply's results are uint8 and the
draw's table is integers and fp64 bit patterns, so every comparison is exact.  The apply kernel has one code path for
every image size (one workgroup per image, intermediates in the global workspace); 224x224x3 is there for an image that
takes many passes of the workgroup."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import randaug_ref as R

SHAPES = [(3, 32, 32, 3), (3, 24, 40, 3), (3, 24, 40, 1)]
FILL = (124, 116, 104)


def dev():
    return torch.device("cuda:0")


def make(C=3, **kw):
    from nvit_amd.randaug import RandAugment
    return RandAugment(fill=FILL if C == 3 else FILL[:1], **kw).to(dev())


def images(B, H, W, C, seed=0):
    """Image 0 random, image 1 low contrast with a channel offset, image 2 random with a constant middle channel."""
    g = np.random.default_rng(1000 * H + W + C + seed)
    x = g.integers(0, 256, (B, H, W, C), dtype=np.uint8)
    if B > 1:
        x[1] = (g.integers(100, 140, (H, W, C)) + np.array([0, 20, -30])[:C]).astype(np.uint8)
    if B > 2:
        x[2, :, :, C // 2] = 77
    return x


def run_u8(ra, x, params):
    p = torch.from_numpy(np.ascontiguousarray(params, dtype=np.int32)).to(dev())
    return ra.apply(torch.from_numpy(x).to(dev()), p, return_u8=True).cpu().numpy()


def same(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape, what
    bad = got != want
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def single_op_cases():
    for name in R.CHOICES:
        if name in R.GEOMETRIC:
            for filt in ("bilinear", "bicubic"):
                for m, neg in ((0, 0), (4.5, 0), (9, 1), (10, 0), (10, 1)):
                    yield (name, m, neg, filt)
        else:
            for m, neg in ((0, 0), (9, 0), (9, 1), (10, 1)):
                yield (name, m, neg)
    for raw in (("Rotate", {"value": 77.7}, "bicubic"), ("Rotate", {"value": -98.6}, "bilinear"),
                ("TranslateX", {"value": 36.3}, "bicubic"), ("TranslateY", {"value": -19.8}, "bilinear"),
                ("SolarizeAdd", {"value": 0}), ("SolarizeAdd", {"value": 128}), ("Posterize", {"value": 0}),
                ("Solarize", {"value": 0}), ("Solarize", {"value": 256})):
        yield raw


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_op_alone_equals_the_restatement(shape):
    B, H, W, C = shape
    ra = make(C)
    x = images(B, H, W, C)
    fill = FILL[:C]
    n = 0
    for case in single_op_cases():
        rows = ra.params_for([[case]] * B, H, W).cpu().numpy()
        got = run_u8(ra, x, rows)
        same(got, R.apply_params(x, rows, fill), case)
        if len(case) > 1 and case[1] == 0 and case[0] in R.GEOMETRIC + R.ENHANCE:
            same(got, x, (case, "is the identity"))
        n += 1
    assert n == 5 * 2 * 5 + 10 * 4 + 9


def test_far_moves_show_the_fill_colour_per_channel():
    B, H, W, C = SHAPES[1]
    ra = make(C)
    x = images(B, H, W, C)
    rows = ra.params_for([[("TranslateX", {"value": 39.0}, "bicubic")]] * B, H, W)
    got = ra.apply(torch.from_numpy(x).to(dev()), rows, return_u8=True).cpu().numpy()
    assert (got[:, :, 1:] == np.array(FILL, dtype=np.uint8)).all()
    same(got, R.apply_params(x, rows.cpu().numpy(), FILL), "translate by W - 1")


CHAINS = [
    [("Rotate", 9, 0, "bicubic"), "Equalize"],
    [("Rotate", 10, 1, "bilinear"), "AutoContrast"],
    [("Rotate", 9, 1, "bicubic"), ("Rotate", 4.5, 0, "bilinear")],
    [None, None],
    [("ShearX", 9, 1, "bicubic"), None, ("Sharpness", 9, 0)],
    [None, ("Color", 9, 1), ("TranslateY", 10, 0, "bilinear")],
    [("TranslateY", 9, 1, "bicubic"), ("Contrast", 9, 0), None, ("Rotate", 9, 0, "bicubic")],
    [None, "Invert", None, ("SolarizeAdd", 9, 0)],
    [("Posterize", 9, 0), ("ShearY", 10, 0, "bilinear"), ("Solarize", 9, 0), "Equalize"],
    [("Brightness", 9, 1)],
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_chains_of_one_to_four_layers_equal_the_restatement(shape):
    from nvit_amd import ops
    B, H, W, C = shape
    ra = make(C)
    x = images(B, H, W, C, seed=1)
    xt = torch.from_numpy(x).to(dev())
    fill = FILL[:C]
    for chain in CHAINS:
        rows = ra.params_for([chain] * B, H, W)
        assert rows.shape[1] == len(chain)
        u8 = ra.apply(xt, rows, return_u8=True)
        same(u8.cpu().numpy(), R.apply_params(x, rows.cpu().numpy(), fill), chain)
        f = ra.apply(xt, rows)
        assert f.dtype == torch.float32 and tuple(f.shape) == (B, C, H, W)
        assert torch.equal(f, ops.normalize_images(u8)), chain
        if all(e is None for e in chain):
            same(u8.cpu().numpy(), x, "all layers off")
            assert torch.equal(f, ops.normalize_images(xt))   # the plain normalise
    # a different chain per image in one launch (padded to four layers)
    mixed = [(CHAINS[i % len(CHAINS)] + [None] * 4)[:4] for i in range(B)]
    rows = ra.params_for(mixed, H, W)
    same(run_u8(ra, x, rows.cpu().numpy()), R.apply_params(x, rows.cpu().numpy(), fill), "mixed")
    other = make(C, mean=0.4, std=0.25)
    u8 = other.apply(xt, rows, return_u8=True)
    assert torch.equal(other.apply(xt, rows), ops.normalize_images(u8, 0.4, 0.25))


@pytest.mark.parametrize("filt", ["bilinear", "bicubic"])
def test_224_square_images(filt):
    from nvit_amd import ops
    B, H, W, C = 2, 224, 224, 3
    ra = make(C)
    x = images(B, H, W, C, seed=2)
    xt = torch.from_numpy(x).to(dev())
    rows = ra.params_for([[("Rotate", 9, 0, filt), "Equalize"], [("ShearX", 10, 1, filt), ("TranslateY", 9, 0, filt)]], H, W)
    u8 = ra.apply(xt, rows, return_u8=True)
    same(u8.cpu().numpy(), R.apply_params(x, rows.cpu().numpy(), FILL), filt)
    assert torch.equal(ra.apply(xt, rows), ops.normalize_images(u8))


DRAWS = [
    dict(),                                                                               # rand-m9-mstd0.5-inc1
    dict(magnitude_std=0.0, increasing=False, prob=1.0, num_layers=1, interpolation="bicubic"),
    dict(magnitude_std=math.inf, magnitude=7.0, num_layers=4, interpolation="bilinear", translate_pct=0.3),
    dict(magnitude_std=2.0, magnitude_max=8.0, increasing=False, num_layers=4),           # the clamp at both ends
    dict(prob=0.0),
]


@pytest.mark.parametrize("kw", DRAWS, ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()) or "defaults")
def test_draw_equals_the_restatement(kw):
    B, first, seed = 300, 2 ** 33 + 5, 0x1234567890ABCDEF
    ra = make(seed=seed, first_index=first, **kw)
    twin = dict(num_layers=kw.get("num_layers", 2), magnitude=kw.get("magnitude", 9.0), mstd=kw.get("magnitude_std", 0.5),
                mmax=kw.get("magnitude_max", 10.0), increasing=kw.get("increasing", True), prob=kw.get("prob", 0.5),
                interpolation=kw.get("interpolation", "random"), translate_pct=kw.get("translate_pct", 0.45))
    for H, W in ((32, 32), (24, 40)):
        ra.load_state_dict({"seed": seed, "step": 0})
        for step in range(3):
            got = ra.draw(B, H, W)
            assert got.dtype == torch.int32 and tuple(got.shape) == (B, twin["num_layers"], R.ROW)
            want = R.draw(seed, step, first, B, H, W, **twin)
            bad = np.argwhere(got.cpu().numpy() != want)
            assert not len(bad), (H, W, step, bad[:4].tolist())
        assert ra.step == 3 and ra.state_dict() == {"seed": seed, "step": 3}
    if kw.get("prob", 0.5) > 0:
        assert (want[:, :, 0] != 0).any()
    else:
        assert not want.any()


def test_batch_split_resume_and_the_call():
    from nvit_amd import ops
    from nvit_amd.randaug import RandAugment
    H, W = 24, 40
    whole = make(seed=5).draw(8, H, W)
    lo, hi = make(seed=5, first_index=0).draw(4, H, W), make(seed=5, first_index=4).draw(4, H, W)
    assert torch.equal(whole, torch.cat([lo, hi]))
    # resume: a fresh object loaded with the state continues the uninterrupted sequence
    a = make(seed=21)
    seq = [a.draw(64, H, W) for _ in range(4)]
    b = make(seed=21)
    b.draw(64, H, W)
    b.draw(64, H, W)
    c = make(seed=0)
    c.load_state_dict(b.state_dict())
    assert torch.equal(c.draw(64, H, W), seq[2]) and torch.equal(c.draw(64, H, W), seq[3])
    d = RandAugment(seed=21, fill=FILL)
    d.load_state_dict({"seed": 21, "step": 3})   # loaded before .to(device)
    assert torch.equal(d.to(dev()).draw(64, H, W), seq[3])
    assert not torch.equal(seq[0], seq[1])
    # the call is the draw, then the apply
    x = images(16, H, W, 3, seed=4)
    e = make(seed=77)
    e.load_state_dict({"seed": 77, "step": 6})
    f = e(torch.from_numpy(x).to(dev()))
    rows = R.draw(77, 6, 0, 16, H, W)
    assert (rows[:, :, 0] != 0).any() and e.step == 7
    want = R.apply_params(x, rows, FILL)
    assert torch.equal(f, ops.normalize_images(torch.from_numpy(want).to(dev())))
