"""GPU tests, op level: nvit_patch_embed_fwd (patch_embed.hip), nvit_im2col (misc.hip) and nvit_shadow_weights
(weights.hip) against the references, bounds and exact expectations of patch_check.py, at the smallest shapes that reach
every edge of the kernels: M below, at and above one 256-token tile and in a second group of 8 tiles, one K stage and a
half-empty one, column tiles of 4 and 8 columns, T = 1, the smallest image, every reflect pad of both gather paths; for
the shadows ragged and sub-tile matrices, every destination combination inside a sentinel-filled stacked buffer and a
table of more work items than the grid has workgroups.  test_patch_check.py shows on the CPU that the bounds pass an
fp32 / bf16 emulation of the kernel and fail the mutants named there.  Run on the MI355X box: pytest -m gpu.

Largest err/bound seen on the MI355X (observations against the fp64 reference; no bound is set from them):
  nvit_patch_embed_fwd   gauss: out_l 0.069, out_g 0.065 (the largest at C = 256 / 252, M = 257)
  identity data, the saved rows, the twins against bf16(out), nvit_im2col and every nvit_shadow_weights result are
  bit-exact: there is no figure to report
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_check as gc
import kohonen_check as kc
import patch_check as pc
from attn_check import Padded, SENTINEL

F32T, BF16T = torch.float32, torch.bfloat16
NAN = float("nan")


def dev():
    return torch.device("cuda:0")


def ops_():
    from nvit_amd import ops
    return ops


def weight_images(c):
    """the split weight images of both sides from nvit_shadow_weights (perm 2), checked against the host layout"""
    ops = ops_()
    from nvit_amd._lib import BF16
    imgs, ent = [], []
    for side in ("l", "g"):
        P, K, w, b, pos = pc.side_of(c, side)
        imgs.append(torch.zeros((w.shape[0], 2 * pc.kp_of(K)), device=dev(), dtype=BF16T))
        ent.append((w.to(dev()), imgs[-1], 2 * pc.kp_of(K), K, None, 0, 0, 2))
    t, n = ops.shadow_table(ent, dev())
    ops.shadow_weights(t, n, BF16)
    for im, side in zip(imgs, ("l", "g")):
        assert gc.bits_equal(im.cpu(), pc.split_image(c["w_" + side]))
    return imgs


def run_patch(c, img, sh, save_rows, twins):
    """nvit_patch_embed_fwd with the image inside NaN margins and every output inside sentinel margins; -> outputs on
    the CPU: out_l, out_g, (save_rows) a_l, a_g [M, Kp], (twins) lo_l, lo_g."""
    ops = ops_()
    B, ch, S, Pl, Pg, C = c["geo"]
    M = c["M"]
    Mpad = ops.round_up(M, pc.TILE_M)
    bufs = {}
    for side, P in (("l", Pl), ("g", Pg)):
        bufs["out_" + side] = Padded((M, C), F32T, SENTINEL)
        bufs["lo_" + side] = Padded((M, C), BF16T, SENTINEL) if twins else None
        bufs["a_" + side] = Padded((Mpad, pc.kp_of(ch * P * P)), BF16T, SENTINEL) if save_rows else None
    d = lambda t: None if t is None else t.to(dev())
    keep = [d(c[k]) for k in ("b_l", "pos_l", "b_g", "pos_g")]
    ptr = lambda p: None if p is None else p.ptr()
    ops.check(ops._lib.load().nvit_patch_embed_fwd(
        img.ptr(), ops._p(sh[0]), ops._p(keep[0]), ops._p(keep[1]), ptr(bufs["out_l"]), ptr(bufs["lo_l"]), ptr(bufs["a_l"]),
        ops._p(sh[1]), ops._p(keep[2]), ops._p(keep[3]), ptr(bufs["out_g"]), ptr(bufs["lo_g"]), ptr(bufs["a_g"]),
        B, ch, S, Pl, Pg, C, ops._s()), "nvit_patch_embed_fwd")
    torch.cuda.synchronize()
    assert img.margins_intact(), "the image's NaN margins changed"
    for k, p in bufs.items():
        assert p is None or p.margins_intact(), f"{k}: written outside the buffer"
    out = {k: p.t.cpu() for k, p in bufs.items() if p is not None}
    for side in ("l", "g"):
        if save_rows:
            out["a_" + side] = out["a_" + side][:M].contiguous()       # (rows >= M of the padded buffer are unspecified)
    return out


@pytest.mark.parametrize("geo", pc.GEOMETRIES, ids=pc.geo_id)
def test_patch_embed_within_fp64_bounds_and_bit_stable(geo):
    B, ch, S, Pl, Pg, C = geo
    for fam in pc.FAMILIES:
        for bias in (True, False):
            c = pc.case(geo, fam, bias=bias)
            img = Padded(tuple(c["img"].shape), F32T, NAN, c["img"].to(dev()))
            sh = weight_images(c)
            twins = C % 8 == 0
            got = run_patch(c, img, sh, True, twins)
            for side in ("l", "g"):
                ref = pc.reference(c, side)
                out = got["out_" + side]
                label = f"patch_embed {pc.geo_id(geo)} {fam} bias={bias} out_{side}"
                if fam == "identity":
                    gc.assert_exact(out, ref["ref_split"], label)
                else:
                    m = kc.check(out, ref["ref_split"], ref["bound"], label, verbose=False)
                    print(f"   {label}: max err/bound {m:.3f}")
                if twins:
                    assert gc.bits_equal(got["lo_" + side], out.bfloat16()), f"{label}: the twin is not bf16(out)"
                    if fam == "gauss":
                        kc.check(got["lo_" + side], ref["ref_split"], ref["bound"], label + " twin", verbose=False)
                K = ref["rows"].shape[1]
                assert gc.bits_equal(got["a_" + side][:, :K].contiguous(), ref["rows"]), f"{label}: saved rows"
                assert (got["a_" + side][:, K:] == 0).all(), f"{label}: saved rows not zero behind K"
            # the outputs do not depend on the saved rows or the twins (the two waits of the stage loop), nor on the run
            plain = run_patch(c, img, sh, False, False)
            again = run_patch(c, img, sh, True, twins)
            for side in ("l", "g"):
                assert gc.bits_equal(plain["out_" + side], got["out_" + side]), f"{fam} out_{side}: save_rows changes the bits"
            assert all(gc.bits_equal(again[k], got[k]) for k in got), f"{fam}: two runs differ"


@pytest.mark.parametrize("B,ch,S,Pl,Pg,C,twins", pc.REJECTED)
def test_patch_embed_and_im2col_reject(B, ch, S, Pl, Pg, C, twins):
    """pad >= S, S % Pl != 0, Pl % 4 != 0, and C % 8 != 0 with twins: an error code, nothing launched."""
    ops = ops_()
    from nvit_amd._lib import F32
    big = lambda dt: torch.zeros(1 << 16, device=dev(), dtype=dt)
    img, f, h = big(F32T), big(F32T), big(BF16T)
    with pytest.raises(RuntimeError):
        ops.check(ops._lib.load().nvit_patch_embed_fwd(
            ops._p(img), ops._p(h), None, ops._p(f), ops._p(f), ops._p(h) if twins else None, None,
            ops._p(h), None, ops._p(f), ops._p(f), ops._p(h) if twins else None, None, B, ch, S, Pl, Pg, C, ops._s()), "patch")
    if not twins:
        with pytest.raises(RuntimeError):
            ops.check(ops._lib.load().nvit_im2col(F32, ops._p(img), ops._p(f), ops._p(f), B, ch, S, Pl, Pg, ops._s()), "im2col")
    torch.cuda.synchronize()
    assert (f == 0).all() and (h == 0).all()


@pytest.mark.parametrize("geo", pc.GEOMETRIES, ids=pc.geo_id)
def test_im2col_exact(geo):
    """fp32: the gathered pixels, bit for bit; bf16: one rounding of them.  The identity image shows a transposed
    (ph, pw) or a mirrored border."""
    ops = ops_()
    from nvit_amd._lib import BF16, F32
    B, ch, S, Pl, Pg, C = geo
    for fam in pc.FAMILIES:
        src = pc.case(geo, fam)["img"]
        img = Padded(tuple(src.shape), F32T, NAN, src.to(dev()))
        want = [pc.patches(src, P, Pl) for P in (Pl, Pg)]
        for dt, td in ((F32, F32T), (BF16, BF16T)):
            outs = [Padded(tuple(w.shape), td, SENTINEL) for w in want]
            ops.check(ops._lib.load().nvit_im2col(dt, img.ptr(), outs[0].ptr(), outs[1].ptr(), B, ch, S, Pl, Pg, ops._s()),
                      "nvit_im2col")
            torch.cuda.synchronize()
            assert img.margins_intact() and all(o.margins_intact() for o in outs)
            for o, w, name in zip(outs, want, ("A_l", "A_g")):
                assert gc.bits_equal(o.t.cpu(), w.to(td)), f"im2col {pc.geo_id(geo)} {fam} {name} {td}"


# ------------------------------------------------------------------------------------------------ weight shadows
def run_shadow(specs, td, fill=SENTINEL):
    """nvit_shadow_weights over one table of `specs`, all sources in one flat buffer and all destinations in one flat
    `fill`-filled buffer laid out by patch_check.shadow_layout; -> (the destination buffer on the CPU, total items)."""
    ops = ops_()
    from nvit_amd._lib import BF16, F32
    od, ot, total = pc.shadow_layout(specs)
    flat = torch.full((total,), fill, device=dev(), dtype=td)
    src = torch.cat([s["src"].reshape(-1) for s in specs]).to(dev())
    ent, o = [], 0
    for s, o_d, o_t in zip(specs, od, ot):
        rows, cols = s["src"].shape
        ent.append((src[o:o + rows * cols].view(rows, cols), flat[o_d:] if s["dst"] else None, s["dst_ld"], s["dst_cols"],
                    flat[o_t:] if s["dstT"] else None, s["dstT_ld"], s["dstT_cols"], s["perm"]))
        o += rows * cols
    table, items = ops.shadow_table(ent, dev())
    assert items == sum(a * b for a, b in map(pc.shadow_items, specs))
    ops.shadow_weights(table, items, F32 if td == F32T else BF16)
    torch.cuda.synchronize()
    return flat.cpu(), items


def shadow_specs(rows, cols, seed=3):
    src = gc.gauss_data((rows, cols), seed)
    return [pc.spec(src, 0, dst=True, dstT=False), pc.spec(src, 0, dst=False, dstT=True), pc.spec(src, 0),
            pc.spec(src, 0, pad_c=7, pad_r=9), pc.spec(src, 0, pad_c=70, pad_r=3, slack=5),
            pc.spec(src, 0, dst=False, pad_r=66, slack=1)]


@pytest.mark.parametrize("td", [F32T, BF16T], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,cols", pc.SHADOW_CASES)
def test_shadow_copy_transpose_padding_inside_a_stacked_buffer(rows, cols, td):
    """dst only, dstT only, both; zero padding to dst_cols / dstT_cols (within the tile and a tile further); leading
    dimensions beyond the written extent; every destination a slice of one sentinel-filled buffer of which only the
    stated extents may change."""
    specs = shadow_specs(rows, cols)
    got, _ = run_shadow(specs, td)
    assert gc.bits_equal(got, pc.shadow_expected(specs, td))


@pytest.mark.parametrize("F", pc.PERM1_F)
def test_shadow_swiglu_interleave(F):
    specs = [pc.spec(gc.gauss_data((2 * F, 40), 5), 1, pad_c=8, pad_r=4), pc.spec(gc.gauss_data((2 * F, 3), 6), 1, dstT=False)]
    for td in (F32T, BF16T):
        got, _ = run_shadow(specs, td)
        assert gc.bits_equal(got, pc.shadow_expected(specs, td))


@pytest.mark.parametrize("K", pc.PERM2_K)
def test_shadow_split_image_leaves_the_padding_alone(K):
    """[hi32 | lo32] slices exact, hi + lo within 2^-16 |w| (test_patch_check.py, from the same expectation), and the
    padding columns of the last slice exactly as allocated: a recognisable fill, not zero."""
    specs = [pc.spec(gc.gauss_data((rows, K), 6) * 0.1, 2, slack=s) for rows, s in zip(pc.PERM2_ROWS, (0, 3))]
    got, _ = run_shadow(specs, BF16T, fill=7.0)
    assert gc.bits_equal(got, pc.shadow_expected(specs, BF16T, fill=7.0))


def test_shadow_table_larger_than_the_grid():
    """4200 entries, more work items than the 4096 workgroups of the launch: the stride loop and the first_item search."""
    specs = pc.big_table()
    got, items = run_shadow(specs, F32T)
    assert len(specs) >= 4200 and items > pc.GRID_CAP
    assert gc.bits_equal(got, pc.shadow_expected(specs, F32T))
    got, _ = run_shadow(specs, BF16T)
    assert gc.bits_equal(got, pc.shadow_expected(specs, BF16T))
