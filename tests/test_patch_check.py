"""The oracles of patch_check.py have teeth (CPU only, no GPU): the gather written from its definition is the oracle's
im2col at every geometry; the fp32 / bf16 emulation of the patch-embedding kernel stays inside the bounds (identity data:
bit-exact) at every geometry, family and bias setting of the GPU test; the split product is within the derived constant
of the true one; every mutant - a way the kernel can go wrong without crashing - is outside a bound or not bit-equal on a
listed case (printed); and the expected weight-shadow buffers are what a restatement of the kernel's table walk leaves."""
import pytest
import torch

import gemm_check as gc
import kohonen_check as kc
import patch_check as pc
from oracle import nvit_oracle as O

F32, BF16 = torch.float32, torch.bfloat16


@pytest.mark.parametrize("geo", pc.GEOMETRIES, ids=pc.geo_id)
def test_gather_is_the_oracle_im2col(geo):
    B, ch, S, Pl, Pg, C = geo
    for fam in pc.FAMILIES:
        img = pc.case(geo, fam)["img"]
        for P in (Pl, Pg):
            want = O.im2col(img, P, Pl, (P - Pl) // 2).reshape(-1, ch * P * P)
            assert gc.bits_equal(pc.patches(img, P, Pl), want)
            padded = pc.patches(img, P, Pl, Kp=pc.kp_of(ch * P * P))
            assert gc.bits_equal(padded[:, :ch * P * P].contiguous(), want) and (padded[:, ch * P * P:] == 0).all()


def test_geometries_are_the_edges_of_the_issue():
    m_of = lambda g: g[0] * (g[2] // g[3]) ** 2
    assert {m_of(g) for g in pc.GEOMETRIES} >= {1, 255, 256, 257, 2049}
    assert {g[5] for g in pc.GEOMETRIES} >= {4, 8, 60, 252, 256, 260, 264, 516}
    ks = {g[1] * P * P for g in pc.GEOMETRIES for P in (g[3], g[4])}
    assert {16, 32, 288} <= ks and pc.kp_of(16) == 32 and pc.kp_of(32) == 32 and pc.kp_of(288) == 288
    assert {(g[4] - g[3]) // 2 for g in pc.GEOMETRIES} >= {0, 2, 4, 6}
    assert -(-2049 // pc.TILE_M) == 9                       # 9 token tiles: two groups of 8
    # every integer of +-65535 is exactly hi + lo
    x = torch.arange(-65535, 65536).float()
    hi, lo = pc.split(x)
    assert torch.equal(hi.float() + lo.float(), x)


def verdict(c, got, refs=None, verbose=False):
    """Raises AssertionError unless `got` (out_l, out_g, a_l, a_g) is what the GPU test accepts for case c."""
    worst = 0.0
    for side in ("l", "g"):
        ref = pc.reference(c, side) if refs is None else refs[side]
        out = got["out_" + side]
        label = f"{pc.geo_id(c['geo'])} {c['family']} out_{side}"
        if c["family"] == "identity":
            assert torch.equal(ref["ref_split"], ref["ref_true"])
            gc.assert_exact(out, ref["ref_split"], label)
        else:
            worst = max(worst, kc.check(out, ref["ref_split"], ref["bound"], label, verbose))
            kc.check(out.bfloat16(), ref["ref_split"], ref["bound"], label + " twin", verbose)   # (half an ulp more)
        K = ref["rows"].shape[1]
        rows = got["a_" + side]
        assert gc.bits_equal(rows[:, :K].contiguous(), ref["rows"]), f"{label}: saved rows differ from bf16(patch)"
        assert (rows[:, K:] == 0).all(), f"{label}: saved rows are not zero behind K"
    return worst


@pytest.mark.parametrize("geo", pc.GEOMETRIES, ids=pc.geo_id)
def test_emulation_inside_the_bounds(geo):
    worst = 0.0
    for fam in pc.FAMILIES:
        for bias in (True, False):
            c = pc.case(geo, fam, bias=bias)
            worst = max(worst, verdict(c, pc.emulate(c)))
    print(f"   {pc.geo_id(geo)}: largest err/bound of the emulation {worst:.3f}")


@pytest.mark.parametrize("geo", pc.GEOMETRIES, ids=pc.geo_id)
def test_split_product_within_the_derived_constant_of_the_true_one(geo):
    c = pc.case(geo, "gauss")
    for side in ("l", "g"):
        ref = pc.reference(c, side)
        ratio = ((ref["ref_split"] - ref["ref_true"]).abs() / ref["mag_true"]).max().item()
        print(f"   {pc.geo_id(geo)} side {side}: |split - true| / sum |a||w| = {ratio * 2 ** 16:.3f} * 2^-16")
        assert ratio <= pc.SPLIT_REL


G = {pc.geo_id(g): g for g in pc.GEOMETRIES}
KILLS = {
    "drop_al_wh": [("B1_ch1_S4_Pl4_Pg4_C4", "gauss"), ("B5_ch3_S32_Pl4_Pg8_C192", "identity")],
    "drop_ah_wl": [("B1_ch1_S4_Pl4_Pg4_C4", "gauss"), ("B2_ch2_S8_Pl4_Pg12_C264", "gauss")],
    "halves_swapped": [("B3_ch1_S8_Pl4_Pg8_C60", "gauss"), ("B5_ch3_S32_Pl4_Pg8_C192", "identity")],
    "symmetric": [("B3_ch1_S8_Pl4_Pg8_C60", "identity"), ("B2_ch2_S8_Pl4_Pg12_C264", "identity"),
                  ("B1_ch1_S8_Pl4_Pg16_C8", "gauss")],
    "reflect_x_only": [("B3_ch1_S8_Pl4_Pg8_C60", "identity"), ("B255_ch1_S4_Pl4_Pg8_C8", "identity")],
    "transposed": [("B1_ch1_S4_Pl4_Pg4_C4", "identity"), ("B2_ch2_S8_Pl4_Pg12_C264", "identity")],
    "pos_by_m": [("B3_ch1_S8_Pl4_Pg8_C60", "identity"), ("B5_ch3_S32_Pl4_Pg8_C192", "gauss")],
    "k_tail": [("B1_ch1_S4_Pl4_Pg4_C4", "identity"), ("B5_ch3_S32_Pl4_Pg8_C192", "gauss")],
    "last_token_tile": [("B257_ch1_S4_Pl4_Pg8_C8", "identity"), ("B2049_ch1_S4_Pl4_Pg4_C8", "gauss")],
    "second_group_first_side": [("B2049_ch1_S4_Pl4_Pg4_C8", "identity"), ("B2049_ch1_S4_Pl4_Pg4_C8", "gauss")],
    "last_column_tile": [("B257_ch1_S4_Pl4_Pg4_C260", "identity"), ("B257_ch1_S4_Pl4_Pg4_C516", "gauss"),
                         ("B1_ch1_S4_Pl4_Pg4_C4", "identity")],
}


def test_every_mutant_is_listed():
    assert set(KILLS) == set(pc.MUTANTS)


@pytest.mark.parametrize("mutant", pc.MUTANTS)
def test_mutant_is_outside_the_bounds_or_not_bit_equal(mutant):
    for gid, fam in KILLS[mutant]:
        c = pc.case(G[gid], fam)
        refs = {s: pc.reference(c, s) for s in ("l", "g")}
        verdict(c, pc.emulate(c), refs)
        with pytest.raises(AssertionError):
            verdict(c, pc.emulate(c, mutant), refs)
        print(f"   {mutant}: shown on {gid} {fam}")


# ------------------------------------------------------------------------------------------------ weight shadows
def shadow_specs(rows, cols, seed=3):
    src = gc.gauss_data((rows, cols), seed)
    return [pc.spec(src, 0, dst=True, dstT=False), pc.spec(src, 0, dst=False, dstT=True), pc.spec(src, 0),
            pc.spec(src, 0, pad_c=7, pad_r=9), pc.spec(src, 0, pad_c=70, pad_r=3, slack=5),
            pc.spec(src, 0, dst=False, pad_r=66, slack=1)]


@pytest.mark.parametrize("rows,cols", pc.SHADOW_CASES)
def test_shadow_expectation_is_what_the_table_walk_leaves(rows, cols):
    for td in (F32, BF16):
        specs = shadow_specs(rows, cols)
        want = pc.shadow_expected(specs, td)
        assert gc.bits_equal(pc.shadow_walk(specs, td), want)
        od, ot, total = pc.shadow_layout(specs)
        assert (want[:5] == pc.SENTINEL).all() and (want[-5:] == pc.SENTINEL).all()
        # entry 3: dst [rows, cols + 7] zero padded, dstT [cols, rows + 9]
        d = want[od[3]:od[3] + rows * (cols + 7)].view(rows, cols + 7)
        assert gc.bits_equal(d[:, :cols].contiguous(), specs[3]["src"].to(td)) and (d[:, cols:] == 0).all()
        t = want[ot[3]:ot[3] + cols * (rows + 9)].view(cols, rows + 9)
        assert gc.bits_equal(t[:, :rows].contiguous(), specs[3]["src"].t().to(td).contiguous()) and (t[:, rows:] == 0).all()


@pytest.mark.parametrize("F", pc.PERM1_F)
def test_perm1_rule(F):
    want = torch.tensor([(s // 32) * 16 + s % 32 if s % 32 < 16 else F + (s // 32) * 16 + (s % 32 - 16) for s in range(2 * F)])
    assert torch.equal(pc.perm1_rows(F), want) and sorted(want.tolist()) == list(range(2 * F))
    specs = [pc.spec(gc.gauss_data((2 * F, 40), 5), 1, pad_c=8, pad_r=4)]
    for td in (F32, BF16):
        assert gc.bits_equal(pc.shadow_walk(specs, td), pc.shadow_expected(specs, td))


@pytest.mark.parametrize("K", pc.PERM2_K)
def test_perm2_split_image(K):
    for rows in pc.PERM2_ROWS:
        w = gc.gauss_data((rows, K), 6) * 0.1
        specs = [pc.spec(w, 2, slack=3)]
        want = pc.shadow_expected(specs, BF16, fill=7.0)
        assert gc.bits_equal(pc.shadow_walk(specs, BF16, fill=7.0), want)
        Kp = pc.kp_of(K)
        img = want[5:5 + rows * (2 * Kp + 3)].view(rows, 2 * Kp + 3)[:, :2 * Kp]
        assert gc.bits_equal(img.contiguous(), pc.split_image(w, fill=7.0))
        sl = img.reshape(rows, Kp // 32, 2, 32)
        hi, lo = sl[:, :, 0].reshape(rows, Kp)[:, :K], sl[:, :, 1].reshape(rows, Kp)[:, :K]
        assert ((hi.double() + lo.double() - w.double()).abs() <= 2.0 ** -16 * w.double().abs()).all()
        assert (sl[:, :, 0].reshape(rows, Kp)[:, K:] == 7.0).all() and (sl[:, :, 1].reshape(rows, Kp)[:, K:] == 7.0).all()


def test_big_table_needs_the_stride_loop_and_the_search():
    specs = pc.big_table()
    assert len(specs) >= 4200
    items = [t[0] * t[1] for t in map(pc.shadow_items, specs)]
    assert sum(items) > pc.GRID_CAP and max(items) > 1 and {s["perm"] for s in specs} == {0, 1}
    od, ot, total = pc.shadow_layout(specs)
    assert total * 4 + sum(s["src"].numel() for s in specs) * 4 < 16 * 2 ** 20
    want = pc.shadow_expected(specs, F32)
    assert gc.bits_equal(pc.shadow_walk(specs, F32), want)
    assert not gc.bits_equal(pc.shadow_walk(specs, F32, stride_loop=False), want)
