"""The checkers of tests/parity_check.py for the post-processing kernels (geometric consistency, multires, image preparation), without a
GPU.  (1) The fp32 CPU oracles as the subject - oracle/fusion_oracle.py evaluates the chain in another order than the kernel (batched
matmuls, torch's grid_sample), torch's own fp32 upsample is another evaluation of the image preparation: no element out of bound, the cap
on the undecidable share holds, the cases are not vacuous.  That validates the derived bounds.  (2) Planted corruptions of a correct
output: each is reported and localised to its view, level, rows or block.  Each test also states, as a fact, whether the criterion the
older tests assert (mismatch fractions and relative L1 sums, restated in ``_old_*``) lets the corruption through at the size of these
cases: it passes the wrong level, the single pixel, a stale block at full size and the multires corner; it sees the corruptions that move
a whole view or a sizeable share of these small images - by a sum, without a location."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import parity_check as pc
import postproc_parity_cases as cs
from conftest import rel_l1

C5, C10 = "67x93-S5", "131x257-S10"


def _old_literal(got, good):
    """tests/test_fusion_gpu.py::test_check_geometric_consistency_matches_reference_capture, with the correct output as the capture."""
    same = got["masks9"][-1] == good["masks9"][-1]
    with np.errstate(all="ignore"):
        return bool((got["masks9"] != good["masks9"]).mean() < 2e-4 and rel_l1(got["xs"], good["xs"]) < 1e-6 and rel_l1(got["ys"], good["ys"]) < 1e-6
                    and rel_l1(got["drep"][same], good["drep"][same]) < 1e-6 and np.abs(got["rel"] - good["rel"]).max() < 1e-5)


def _old_vote(geo, est, good):
    """tests/test_fusion_gpu.py::test_fused_vote_equals_per_view_api_and_oracle: (geo != oracle).mean() < 5e-4, rel_l1(est) < 1e-5."""
    return bool((geo != good["geo_mask"]).mean() < 5e-4 and rel_l1(est, good["depth_est"]) < 1e-5)


@pytest.fixture(scope="module")
def good5():
    return cs.geo_oracle_outputs(C5)


def _kw(out, *names):
    return {k: out[k] for k in (names or ("xs", "ys", "rel", "drep", "masks9", "geo_mask", "depth_est"))}


# ---------------------------------------------------------------- 1. the oracles as the subject
@pytest.mark.parametrize("cid", cs.GEO_IDS)
def test_fusion_oracle_is_within_the_derived_bound(cid):
    ref, S = cs.geo_ref(cid), cs.geo_case(cid)["S"]
    rep = pc.check_geo(ref, f"fusion oracle {cid}", **_kw(cs.geo_oracle_outputs(cid)))
    assert rep.ok, rep.message()
    over = {k: v for k, v in rep.undecidable.items() if v > cs.UNDECIDABLE_CAP}
    assert not over, f"{cid}: undecidable share above {cs.UNDECIDABLE_CAP:.0%}: {over}"
    assert set(rep.checked) == {"xs", "ys", "rel", "drep", "masks9", "geo_mask", "depth_est"}
    # non-vacuity, on the reference alone
    cen = pc.geo_census(ref)
    assert all(cs.BOTH_OUTCOMES <= t <= 1 - cs.BOTH_OUTCOMES for t in cen["true_share"]), cen["true_share"]
    assert cen["rim_share"] >= cs.RIM_SHARE
    if S >= 2:                                               # (S = 1: n = 2, the rule i < n never fires - nothing can be lit by a lower level)
        assert cen["lit_by_lower"] > 0
    else:
        assert cen["lit_by_lower"] == 0


def test_special_values_take_their_paths():
    """The special case: NaN, zero and negative reference pixels and a NaN block / a zero band in source views reach the reference's
    NaN-for-sure, rel = +inf and negative-rel paths, and stay decided."""
    ref, c = cs.geo_ref("67x93-S5-special"), cs.geo_case("67x93-S5-special")
    d = c["depth_ref"].numpy()
    assert np.isnan(d).sum() > 20 and (d == 0).sum() > 20 and (d < 0).sum() > 20
    assert ref["nan_in"][0].sum() == np.isnan(d).sum() and (ref["nan"] & ~ref["nan_in"]).sum() > 50            # NaN taps of the source block
    assert np.isposinf(ref["rel"][0][:, d == 0]).all()
    neg = (d < 0)[None] & ~ref["nan"]
    assert neg.sum() > 100 and (ref["rel"][0][neg] + ref["rel"][1][neg] < 0).all()                              # a negative rel: rel < t holds
    assert not ref["m_hi"][:, :, np.isnan(d) | (d == 0)].any()
    out = cs.geo_oracle_outputs("67x93-S5-special")
    assert np.isnan(out["xs"][:, np.isnan(d)]).all() and np.isnan(out["depth_est"][np.isnan(d)]).all()


# ---------------------------------------------------------------- 2. planted corruptions: geometric consistency
def test_mask_level_with_the_next_threshold(good5):
    """One level thresholded with (i + 1) instead of i: 1e-3 of one level's elements."""
    ref, lv = cs.geo_ref(C5), 3
    g = good5["masks9"].copy()
    g[lv] = g[lv + 1]
    assert (g[lv] != good5["masks9"][lv]).sum() > 0
    rep = pc.check_geo(ref, "level", masks9=g)
    assert not rep.ok and rep.only("masks9", "levels") == lv and "confined to level 3" in rep.message()
    assert _old_literal(dict(good5, masks9=g), good5)                        # the older criterion lets it through


def test_view_sampled_one_texel_to_the_right(good5):
    ref, c, v = cs.geo_ref(C5), cs.geo_case(C5), 2
    src = c["depth_src"].clone()
    src[v, :, :-1] = c["depth_src"][v, :, 1:]
    src[v, :, -1] = 0.0                                      # sample(img, x + 1, y) == sample(img shifted left, x, y), zeros beyond
    bad = cs.geo_oracle_outputs(C5, depth_src=src)
    rep = pc.check_geo(ref, "shifted view", **_kw(bad))
    assert not rep.ok and {"rel", "drep"} <= set(rep.fails)
    assert all(rep.only(k, "views") == v for k in ("rel", "drep", "masks9") if k in rep.fails) and "confined to view 2" in rep.message()
    assert "xs" not in rep.fails and "ys" not in rep.fails
    assert not _old_literal(bad, good5)                    # (the older criterion sees this one, as a sum)


def test_border_clamp_instead_of_zero_padding(good5):
    ref = cs.geo_ref(C5)
    bad = cs.geo_oracle_outputs(C5, padding_mode="border")
    rep = pc.check_geo(ref, "border clamp", **_kw(bad))
    assert not rep.ok and "rel" in rep.fails
    for k in ("rel", "drep"):
        idx = rep.fails[k]["index"]
        assert ref["rim"][idx[:, 0], idx[:, 1], idx[:, 2]].all()               # only samples whose footprint reaches the padding
    assert not _old_literal(bad, good5)                    # (the older criterion sees this one, as a sum)


def test_depth_sum_without_the_gate(good5):
    ref, c = cs.geo_ref(C5), cs.geo_case(C5)
    cnt = good5["masks9"][8].astype(np.float32).sum(0)
    est = ((good5["drep_raw"].sum(0, dtype=np.float32) + c["depth_ref"].numpy()) / (cnt + 1)).astype(np.float32)
    rep = pc.check_geo(ref, "ungated dsum", depth_est=est)
    assert not rep.ok and set(rep.fails) == {"depth_est"}
    gated_off = (~ref["m_hi"][8]).any(0).reshape(-1)
    assert gated_off[rep.fails["depth_est"]["pixels"]].all()                   # only pixels with a view outside m10
    assert rep.fails["depth_est"]["n"] >= 0.9 * (gated_off & ref["est_ok"].reshape(-1)).sum()
    assert not _old_vote(good5["geo_mask"], est, good5)                    # (the older criterion sees this one, as a sum)


def test_vote_rule_with_greater_than(good5):
    ref, c = cs.geo_ref(C5), cs.geo_case(C5)
    geo, est = cs.vote_from_masks(good5["masks9"], good5["drep"], c["depth_ref"].numpy(), cmp_ge=False)
    rep = pc.check_geo(ref, "vote >", geo_mask=geo, depth_est=est)
    assert not rep.ok and set(rep.fails) == {"geo_mask"}
    n = 1 + c["S"]
    exact = np.logical_or.reduce([ref["cnt_lo"][i - 2] == i for i in range(2, n)]).reshape(-1)
    assert exact[rep.fails["geo_mask"]["pixels"]].all()                        # only pixels where some count sits on its level
    assert not _old_vote(geo, est, good5)                    # (the older criterion sees this one, as a sum)


def test_vote_loop_run_to_n_is_the_same_program():
    """``i <= n`` adds the test cnt[n - 2] >= n, which S = n - 1 views cannot meet: for S < 10 the outputs are the same and no check of
    outputs can tell the two apart (for S = 10 it reads a tenth counter that does not exist).  Stated here so that the gap is on record."""
    for cid in ("37x51-S1", "37x51-S2", C5):
        c, out = cs.geo_case(cid), cs.geo_oracle_outputs(cid)
        a = cs.vote_from_masks(out["masks9"], out["drep"], c["depth_ref"].numpy())
        b = cs.vote_from_masks(out["masks9"], out["drep"], c["depth_ref"].numpy(), upto=c["S"] + 2)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], out["geo_mask"])


def test_block_left_at_its_sentinel():
    """One 256-pixel block keeps 0xFF / NaN: 7.6e-3 of this image, 1.4e-4 of a 1184 x 1600 one - below the 5e-4 / 2e-3 the older tests allow."""
    ref, good = cs.geo_ref(C10), cs.geo_oracle_outputs(C10)
    b = 77
    geo, est = good["geo_mask"].copy(), good["depth_est"].copy()
    geo.reshape(-1)[b * 256:(b + 1) * 256] = 0xFF
    est.reshape(-1)[b * 256:(b + 1) * 256] = np.nan
    rep = pc.check_geo(ref, "sentinel block", geo_mask=geo, depth_est=est)
    assert not rep.ok and rep.only("geo_mask", "blocks") == b and rep.only("depth_est", "blocks") == b
    assert rep.fails["geo_mask"]["n"] == 256 and "confined to block 77" in rep.message()
    assert 256 / (1184 * 1600) < 5e-4                      # at full size the older criterion lets it through; at this size:
    assert not bool((geo != good["geo_mask"]).mean() < 5e-4)                    # (the older criterion sees this one, as a sum)


def test_single_wrong_pixel_in_the_last_row(good5):
    ref, c = cs.geo_ref(C5), cs.geo_case(C5)
    H, W = c["H"], c["W"]
    ok = (ref["geo_lo"] == ref["geo_hi"])[H - 1] & ref["est_ok"][H - 1]
    x = int(np.flatnonzero(ok)[len(np.flatnonzero(ok)) // 2])
    geo, est = good5["geo_mask"].copy(), good5["depth_est"].copy()
    geo[H - 1, x] ^= 1
    est[H - 1, x] *= np.float32(1.001)
    rep = pc.check_geo(ref, "one pixel", geo_mask=geo, depth_est=est)
    assert not rep.ok and rep.fails["geo_mask"]["n"] == 1 and rep.fails["depth_est"]["n"] == 1
    assert rep.only("geo_mask", "rows") == H - 1 and rep.only("depth_est", "rows") == H - 1 and "(the last row)" in rep.message()
    assert list(rep.fails["geo_mask"]["pixels"]) == [(H - 1) * W + x]
    assert _old_vote(geo, est, good5)                        # the older criterion lets it through


# ---------------------------------------------------------------- 3. image preparation
def _torch_prep(chw, geom):
    H2, W2, y0, x0, H, W = geom
    return F.interpolate(chw[None], [H2, W2], mode="bilinear", align_corners=True)[0][:, y0:y0 + H, x0:x0 + W]


@pytest.mark.parametrize("form", cs.PREP_FORMS)
@pytest.mark.parametrize("case", cs.PREP_CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}-{c[3]}".replace(" ", ""))
def test_torch_fp32_upsample_is_within_the_prep_bound(case, form):
    H0, W0, rescale, crop = case
    geom = cs.prep_geometry(H0, W0, rescale, crop)
    _, chw = cs.prep_image(H0, W0, form)
    ref, mag = pc.prep_ref64(chw.numpy(), *geom)
    rep = pc.check_prep(_torch_prep(chw, geom), ref, mag, f"torch fp32 {case} {form}")
    assert rep.ok, rep.message()
    if (geom[0], geom[1]) == (H0, W0):
        assert np.array_equal(ref, chw[:, geom[2]:geom[2] + geom[4], geom[3]:geom[3] + geom[5]].double().numpy())


def test_prep_cases_cover_the_store_paths():
    widths = {cs.prep_geometry(*c)[5] % 4 for c in cs.PREP_CASES}
    assert widths == {0, 1, 2, 3}                            # the 16-byte store and every length of the scalar tail
    assert any(cs.prep_geometry(*c)[0] == 1 for c in cs.PREP_CASES) and any(cs.prep_geometry(*c)[1] == 1 for c in cs.PREP_CASES)     # scale = 0


def _prep_good(case, form):
    H0, W0, rescale, crop = case
    geom = cs.prep_geometry(H0, W0, rescale, crop)
    _, chw = cs.prep_image(H0, W0, form)
    ref, mag = pc.prep_ref64(chw.numpy(), *geom)
    return chw, geom, ref, mag, _torch_prep(chw, geom).clone()


def test_prep_last_column_clamp_off_by_one():
    """The last output column reads source column W0 - 2 where it must read W0 - 1."""
    chw, geom, ref, mag, got = _prep_good((67, 93, 2, None), "f32")
    wrong = chw.clone()
    wrong[:, :, -1] = chw[:, :, -2]
    got[:, :, -1] = torch.from_numpy(pc.prep_ref64(wrong.numpy(), *geom)[0][:, :, -1]).float()
    rep = pc.check_prep(got, ref, mag, "last column")
    assert not rep.ok and set(rep.cols) == {geom[5] - 1} and rep.n_fail > geom[4]
    OLD = rel_l1(got, torch.from_numpy(ref)) <= 1e-6         # the older bar (tests/test_scan_gpu.py) sees this one: 1 / 186 of a noise image
    assert not OLD


def test_prep_bgr_swap_missing_on_one_row():
    chw, geom, ref, mag, got = _prep_good((67, 93, 1.37, (88, 120)), "u8bgr")
    r = geom[4] - 1
    got[:, r] = got.flip(0)[:, r].clone()
    rep = pc.check_prep(got, ref, mag, "bgr row")
    assert not rep.ok and rep.only_row() == r and set(rep.channels) == {0, 2} and "(the last row)" in rep.message()


def test_prep_one_corner_tap_wrong():
    """Output (0, 0) takes source texel (0, 1): three elements of 70 000, 4e-6 of the image's L1 sum for a smooth image, named here."""
    chw, geom, ref, mag, got = _prep_good((67, 93, 2, None), "u8")
    got[:, 0, 0] = chw[:, 0, 1]
    rep = pc.check_prep(got, ref, mag, "corner")
    assert not rep.ok and rep.n_fail == 3 and set(rep.rows) == {0} and set(rep.cols) == {0}


# ---------------------------------------------------------------- 4. multires
@pytest.mark.parametrize("shapes", cs.MR_SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_multires_cases_take_both_branches_and_keep_special_values(shapes):
    from oracle import multires_oracle as M
    s1, s2 = shapes
    a, b = cs.mr_maps(s1, s2)
    with np.errstate(all="ignore"):
        out = M.merge(a, b, cs.MR_TH, 1)
        big = M.resize_linear(a, s2)
    took = pc.bits_equal(out, b) & ~pc.bits_equal(big, b)
    assert 0.1 < took.mean() < 0.9
    assert pc.bits_equal(np.where(took, big, out), big).all()                  # everything not taken from scale 2 is the scale-1 value, exactly
    if s1 == s2:
        sp = ~np.isfinite(a)
        assert np.isnan(a).sum() > 5 and np.isposinf(a).sum() > 5 and np.isneginf(a).sum() > 2 and pc.bits_equal(out[sp], a[sp]).all()
    if s1[0] * s1[1] > 4:
        assert (a == 0).sum() > 0 and (a < 0).sum() > 0 and (out <= 0).sum() > 0


def test_multires_one_corner_tap_wrong():
    """The last element one ulp off - what a wrong weight in one corner does: far inside the 1e-6 relative band and the 1e-3 flip share of
    tests/test_multires.py, one element of the bit comparison."""
    from oracle import multires_oracle as M
    a, b = cs.mr_maps((37, 53), (74, 106))
    want = M.merge(a, b, cs.MR_TH, 2)
    got = want.copy()
    got[-1, -1] = np.nextafter(got[-1, -1], np.float32(np.inf))
    flips = np.abs(got - want) > 1e-6 * np.abs(want)
    assert flips.mean() < 1e-3 and rel_l1(got, want) < 1e-4                    # the older criteria pass
    eq = pc.bits_equal(got, want)
    assert (~eq).sum() == 1 and not eq[-1, -1]
    assert pc.bits_equal(np.float32([np.nan, -np.nan, 0.0]), np.float32([-np.nan, np.nan, -0.0])).tolist() == [True, True, False]
