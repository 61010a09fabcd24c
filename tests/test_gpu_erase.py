"""GPU: the on-device RandomErasing (nvit_erase_draw / nvit_erase_apply, nvit_amd/crop.py) against the numpy restatement
tests/crop_ref.py, bit for bit: the draw, and the apply in both modes, in place and out of place.  The train step with
the erasing in its chain is covered by tests/test_gpu_crop.py; tests/test_crop_ref.py pins the noise table."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import crop_ref as R

ASPECT = (0.3, 1 / 0.3)


def dev():
    return torch.device("cuda:0")


def qtab():
    from nvit_amd.crop import normal_quantile_table
    return np.array(normal_quantile_table(), dtype=np.float64).astype(np.float32)


@pytest.mark.parametrize("first", [0, 1000])
def test_draw_equals_the_restatement_and_the_counter_advances(first):
    from nvit_amd.crop import RandomErasing, aspect_table
    ons = 0
    for (H, W), kw in (((16, 16), {"prob": 1.0}), ((8, 12), {"prob": 0.5}), ((224, 224), {}), ((16, 16), {"prob": 0.0}),
                       ((32, 32), {"prob": 1.0, "area": (0.5, 1.0), "aspect": (0.5, 4.0)})):
        e = RandomErasing(seed=2 ** 35 + 3, first_index=first, **kw).to(dev())
        for step in range(3):
            got = e.draw(33, H, W).cpu().numpy()
            want = R.erase_draw(2 ** 35 + 3, step, first, 33, H, W, kw.get("prob", 0.25), kw.get("area", (0.02, 1 / 3)),
                                aspect_table(*kw.get("aspect", ASPECT)))
            assert np.array_equal(got, want), (H, W, kw, step, np.argwhere(got != want)[:4])
            assert e.step == step + 1
            ons += int(want[:, 0].sum())
        assert e.state_dict() == {"seed": 2 ** 35 + 3, "step": 3}
    assert ons > 100
    a = RandomErasing(seed=4).to(dev())
    a.draw(8, 32, 32)
    b = RandomErasing(seed=0).to(dev())
    b.load_state_dict(a.state_dict())
    assert torch.equal(a.draw(8, 32, 32), b.draw(8, 32, 32))


def boxes_for(H, W):
    """Touching every edge, unaligned to 4 columns on either side, one element, one row, one column, the whole image, none."""
    return [(0, 0, 3, 5), (H - 3, W - 5, 3, 5), (0, W - 6, H, 6), (H - 2, 0, 2, W), (2, 1, 4, 6), (1, 2, 3, 5), (3, 3, 2, 1),
            (1, 5, 1, 2), (2, 0, 1, W), (0, 7, H, 1), (0, 0, H, W), None, (H - 1, 0, 2, 2), (0, 0, 0, 4)]


@pytest.mark.parametrize("shape", [(3, 16, 16), (1, 8, 12)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", ["const", "pixel"])
def test_apply_equals_the_restatement_out_of_place_and_in_place(mode, shape):
    from nvit_amd.crop import RandomErasing
    C, H, W = shape
    boxes = boxes_for(H, W)
    B = len(boxes)
    e = RandomErasing(mode=mode).to(dev())
    x = np.random.default_rng(H + W).standard_normal((B, C, H, W)).astype(np.float32)
    xd = torch.from_numpy(x).to(dev())
    table = e.params_for(boxes, keys=[2 ** 40 * (b + 1) + 17 * b for b in range(B)])
    want = R.erase_apply(x, table.cpu().numpy(), mode, qtab())
    got = e.apply(xd, table)
    assert got.data_ptr() != xd.data_ptr() and torch.equal(xd.cpu(), torch.from_numpy(x)), "input modified"
    bad = [boxes[b] for b in range(B) if not np.array_equal(got[b].cpu().numpy().view(np.int32), want[b].view(np.int32))]
    assert not bad, (mode, shape, bad)
    buf = xd.clone()
    same = e.apply(buf, table, inplace=True)
    assert same.data_ptr() == buf.data_ptr() and torch.equal(buf, got), "in place"
    # the last two rows (a box that leaves the image, an empty box) and the None erase nothing
    for b in (B - 1, B - 2, boxes.index(None)):
        assert np.array_equal(want[b], x[b])
    assert (want[0, :, :3, :5] == 0).all() if mode == "const" else (want[0, :, :3, :5] != x[0, :, :3, :5]).all()


def test_call_is_draw_then_apply():
    from nvit_amd.crop import RandomErasing, aspect_table
    x = np.random.default_rng(8).standard_normal((16, 3, 32, 32)).astype(np.float32)
    xd = torch.from_numpy(x).to(dev())
    e = RandomErasing(prob=0.75, seed=13).to(dev())
    e.load_state_dict({"seed": 13, "step": 5})
    table = R.erase_draw(13, 5, 0, 16, 32, 32, 0.75, (0.02, 1 / 3), aspect_table(*ASPECT))
    assert 0 < table[:, 0].sum() < 16
    out = e(xd)
    assert np.array_equal(out.cpu().numpy().view(np.int32), R.erase_apply(x, table, "pixel", qtab()).view(np.int32))
    assert e.step == 6 and torch.equal(xd.cpu(), torch.from_numpy(x))
    again = e(xd.clone(), inplace=True)
    assert not torch.equal(again, out)   # the next step's boxes
