"""The checks of tests/test_wide_parity_gpu.py on an fp32 EMULATION of the wide-range loop's launches, clean and with planted corruptions;
the numpy restatement of the split32 layout against the documented layout; the fp32-oracle yardstick of every cost-volume walk case.  CPU only.

The emulation computes every launch of one ``_WideLoop.step`` (f16x3 form: split32 activations) with torch float32 on a 13 x 101 image - 4 x
32 tiles partial on both axes, interior tiles, and the interior tile row at ty0 = 8 whose 9 x 9 disparity window leaves the image at the
bottom - and each launch is judged by the very reference and bound functions the GPU module applies (``parity_check.wide_*``), from the
tensors that launch read.  The clean emulation passes; then one corruption at a time is planted into one launch's output, and for each the
test asserts that the per-element check fails and names the place, and states what the criteria the suite had before make of it when they
are applied to that launch as the existing kernel tests apply them to theirs (most of these launch forms - GATES / GRU / DELTA on split32
tensors, in place - no kernel test ran at all; only the end-to-end means saw them):
rel_l1 < 2e-6 (test_conv3x3_matches_torch, test_conv3x3_collapsed_disparity_tiles), rel_l1 < 1e-6 on a split32 round trip
(test_conv3x3_split32_layout), rel_l1 < 1e-5 on the hidden state and the disparity update (test_update_block_matches_reference_capture),
max|err| < 5e-6 max|ref| (test_conv3x3_collapsed_disparity_tiles) and, for the walk, max|err| <= 4e-6 max(|vol|, 1)
(test_cost_lines_matches_walk).  ``OLD_CRITERIA_PASS`` is that record: on a 13 x 101 image, where a tile is a tenth of the pixels, the means
see six of the seven corruptions - as one number over the image, naming neither tile, row, pixel nor channel - and the wrong last row not at all.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import parity_check as pc
import wide_parity_cases as cases
from conftest import rel_l1
from test_oracle_golden import hashed

H, W = 13, 101
P = H * W
KW = dict(h=H, w=W, tile=pc.WIDE_TILE)
TILE = (2, 1)                                            # an interior tile: rows 8 .. 11, columns 32 .. 63 (its 9 x 9 windows leave the image below)

# What the criteria the suite had before this module make of each planted corruption: True = they pass it (the corruption is invisible to
# them), False = they fail, as a sum over the image that names no place.  Asserted below, corruption by corruption.
OLD_CRITERIA_PASS = {
    "wrong_tile": False,                                 # rel_l1 2.3e-5 against the 2e-6 bar: one tile is a tenth of this image
    "wrong_last_row": True,                              # rel_l1 1.8e-6 < 2e-6: INVISIBLE
    "split32_hi_lo_swapped": False,                      # rel_l1 5.2e-4
    "gru_reads_updated_h": False,                        # rel_l1 4.1e-2 against 1e-5
    "tap_plane_shifted": False,                          # rel_l1 0.27 on the disparity update
    "collapsed_window_ignores_bottom_padding": False,    # rel_l1 1.3e-3 on z
    "walk_sample_one_texel_off": False,                  # 0.22 against 4e-6: seen as a maximum
}


def img(t):
    return t.view(H, W, -1)


def tile_mask(ty, tx):
    m = torch.zeros(H, W, dtype=torch.bool)
    m[ty * 4:ty * 4 + 4, tx * 32:tx * 32 + 32] = True
    return m.reshape(-1)


def conv32(x, wt, b=None):
    return pc.plain(F.conv2d(pc.nchw(x, H, W).float(), wt, b, padding=1))


def through_split32(t):
    """What a consumer reads back after a producer wrote ``t`` with out_split."""
    return torch.from_numpy(pc.split32_inverse_np(pc.split32_np(t.numpy())))


def disp_features32(d, pad_bottom_replicate=False):
    """100 * (unfold7x7(d) - d) in fp32 [P, 49]; ``pad_bottom_replicate``: the rows below the image repeat the last row instead of being
    zero (the planted error of a collapsed window that ignores the unfold's zero padding at the bottom rim)."""
    dd = d.view(1, 1, H, W)
    p = F.pad(dd, (3, 3, 3, 3))
    if pad_bottom_replicate:
        p[:, :, H + 3:, 3:W + 3] = dd[:, :, H - 1:H, :]
    u = F.unfold(p, [7, 7]).view(1, 49, H, W)
    return pc.plain(100.0 * (u - dd))


@pytest.fixture(scope="module")
def emu():
    """One emulated iteration: weights, the tensors every launch read and wrote (fp32), as a dict."""
    ci = cases.loop_inputs(H, W, 0)
    e = dict(disp=ci["disp"])
    wt = lambda shape, seed, a=0.05: hashed(shape, 4200 + seed, -a, a)
    e["w_corr2"], e["b_corr2"] = wt((64, 64, 3, 3), 1), wt((64,), 2, 0.1)
    e["w_zr"], e["w_q"] = wt((128, 177, 3, 3), 3), wt((64, 177, 3, 3), 4)
    e["w_d1"], e["b_d1"], e["w_d2"], e["b_d2"] = wt((256, 64, 3, 3), 5), wt((256,), 6, 0.1), wt((1, 256, 3, 3), 7), 0.0173
    e["hzr"], e["hq"] = hashed((P, 128), 4210, -0.3, 0.3), hashed((P, 64), 4211, -0.3, 0.3)       # (stand for the hoisted terms)
    e["c1"] = through_split32(torch.relu(hashed((P, 64), 4212, -1.0, 2.0)))                        # (stands for the lookup's output)
    e["h"] = through_split32(ci["net"])
    e["c2"] = through_split32(torch.relu(conv32(e["c1"], e["w_corr2"], e["b_corr2"])))
    e["feat"] = disp_features32(e["disp"])
    e["pre_zr"] = conv32(torch.cat([e["h"], e["feat"], e["c2"]], 1), e["w_zr"]) + e["hzr"]
    e["z"] = torch.sigmoid(e["pre_zr"][:, :64])
    e["rh"] = through_split32(torch.sigmoid(e["pre_zr"][:, 64:]) * e["h"])
    e["pre_q"] = conv32(torch.cat([e["rh"], e["feat"], e["c2"]], 1), e["w_q"]) + e["hq"]
    e["new"] = through_split32((1 - e["z"]) * e["h"] + e["z"] * torch.tanh(e["pre_q"]))
    hid = torch.relu(conv32(e["new"], e["w_d1"], e["b_d1"]))
    proj = e["w_d2"][0].reshape(2, 128, 9)
    e["T"] = torch.cat([hid[:, hf * 128:(hf + 1) * 128] @ proj[hf] for hf in range(2)], 1)          # [P, 18], column = half * 9 + tap
    planes = F.pad(e["T"].t().reshape(2, 9, H, W), (1, 1, 1, 1))
    s = sum(planes[:, tap, tap // 3:tap // 3 + H, tap % 3:tap % 3 + W].sum(0) for tap in range(9)).reshape(-1)
    e["disp_new"] = e["disp"] + 0.01 * (s + e["b_d2"])
    return e


def check(e, launch, **replace):
    """The GPU module's check of one launch on the emulated tensors (``replace``: corrupted outputs) -> ParityReport(s)."""
    g = dict(e, **replace)
    d = lambda k: g[k].double()
    dfeat, dmag = pc.disp_feature_parts(d("disp"), H, W)
    if launch == "corr2":
        pre, mag, a = pc.wide_conv_parts(d("c1"), d("c1").abs(), e["w_corr2"], e["b_corr2"], H, W)
        ref, mag, a = pc.wide_relu_parts(pre, mag, a, True)
        return pc.check_elementwise(d("c2"), ref, mag, pc.WIDE_C, a, "corr2", **KW)
    if launch == "zr":
        pre, mag, a = pc.wide_conv_parts(torch.cat([d("h"), dfeat, d("c2")], 1), torch.cat([d("h").abs(), dmag, d("c2").abs()], 1),
                                         e["w_zr"], None, H, W, init=d("hzr"))
        zp, rp = pc.wide_gates_parts(pre, mag, a, d("h"), True)
        return (pc.check_elementwise(d("z"), zp[0], zp[1], pc.WIDE_C, zp[2], "z|r: z", **KW),
                pc.check_elementwise(d("rh"), rp[0], rp[1], pc.WIDE_C, rp[2], "z|r: r*h", **KW))
    if launch == "q":
        pre, mag, a = pc.wide_conv_parts(torch.cat([d("rh"), dfeat, d("c2")], 1), torch.cat([d("rh").abs(), dmag, d("c2").abs()], 1),
                                         e["w_q"], None, H, W, init=d("hq"))
        ref, mag, a = pc.wide_gru_parts(pre, mag, a, d("z"), d("h"), True)
        return pc.check_elementwise(d("new"), ref, mag, pc.WIDE_C, a, "q / GRU blend", **KW)
    if launch == "delta":
        pre, mag, a = pc.wide_conv_parts(d("new"), d("new").abs(), e["w_d1"], e["b_d1"], H, W)
        ref, mag, a = pc.wide_delta_parts(pre, mag, a, e["w_d2"])
        return pc.check_elementwise(d("T"), ref, mag, pc.WIDE_C, a, "delta head", **KW)
    if launch == "delta_sum":
        ref, mag = pc.delta_sum64(d("T").t().reshape(2, 9, P), e["b_d2"], d("disp"), H, W)
        return pc.check_elementwise(d("disp_new"), ref, mag, pc.C_DSUM, 0.0, "delta_sum", **KW)
    raise ValueError(launch)


def ref64(e, key):
    """The float64 value of an emulated output from the same inputs (what the old mean criteria compared with)."""
    d = lambda k: e[k].double()
    dfeat, _ = pc.disp_feature_parts(d("disp"), H, W)
    if key == "c2":
        return torch.relu(pc.conv_ref(d("c1"), d("c1").abs(), e["w_corr2"], e["b_corr2"], H, W)[0])
    if key in ("z", "rh"):
        pre = pc.conv64(torch.cat([d("h"), dfeat, d("c2")], 1), e["w_zr"], H, W) + d("hzr")
        return torch.sigmoid(pre[:, :64]) if key == "z" else torch.sigmoid(pre[:, 64:]) * d("h")
    if key == "new":
        pre = pc.conv64(torch.cat([d("rh"), dfeat, d("c2")], 1), e["w_q"], H, W) + d("hq")
        return (1 - d("z")) * d("h") + d("z") * torch.tanh(pre)
    raise ValueError(key)


def test_the_clean_emulation_passes_every_check(emu):
    interior = pc.wide_interior_tiles(H, W)
    assert bool(interior[TILE]) and bool(interior.any()) and not bool(interior.all())
    assert not any(bool(pc.wide_interior_tiles(h, w).any()) for h, w in cases.SHAPES if (h, w) not in cases.WITH_INTERIOR)
    assert all(bool(pc.wide_interior_tiles(h, w).any()) and not bool(pc.wide_interior_tiles(h, w).all()) for h, w in cases.WITH_INTERIOR)
    for launch in ("corr2", "zr", "q", "delta", "delta_sum"):
        reps = check(emu, launch)
        for rep in (reps if isinstance(reps, tuple) else (reps,)):
            assert rep.ok and rep.max_ratio < 1.0, rep.message()
    for key in ("c2", "z", "rh", "new"):                   # ... and the old criteria, of course
        assert rel_l1(emu[key], ref64(emu, key)) < 1e-6


def test_one_wrong_tile(emu):
    """corr2: one 4 x 32 tile lost the weights' lo halves (x * w_lo never accumulated): 2^-12 relative per product."""
    bad = through_split32(torch.relu(conv32(emu["c1"], emu["w_corr2"].half().float(), emu["b_corr2"])))
    m = tile_mask(*TILE)
    got = torch.where(m[:, None], bad, emu["c2"])
    rep = check(emu, "corr2", c2=got)
    assert not rep.ok and rep.only_tile() == TILE and "confined to tile (2, 1)" in rep.message()
    ref = ref64(emu, "c2")
    old_pass = rel_l1(got, ref) < 2e-6                    # (test_conv3x3_matches_torch: all a RELU launch was held to)
    assert old_pass == OLD_CRITERIA_PASS["wrong_tile"], rel_l1(got, ref)


def test_a_wrong_last_row(emu):
    """corr2: the last image row lost the bias' low bits (a bias added in f16): <= 2^-12 of |bias| on 1 / 13 of the pixels."""
    got = emu["c2"].clone()
    pre = conv32(emu["c1"], emu["w_corr2"], None) + emu["b_corr2"].half().float()
    img(got)[H - 1] = img(through_split32(torch.relu(pre)))[H - 1]
    rep = check(emu, "corr2", c2=got)
    assert not rep.ok and rep.only_row() == H - 1 and "(the last row)" in rep.message()
    ref = ref64(emu, "c2")
    old_pass = rel_l1(got, ref) < 2e-6
    assert 0 < rel_l1(got, ref) and old_pass == OLD_CRITERIA_PASS["wrong_last_row"], rel_l1(got, ref)


def test_hi_and_lo_swapped_in_one_chunk_of_one_pixel(emu):
    """corr2's split32 output: the 32 hi and the 32 lo halves of channels 32 .. 63 of one pixel change places."""
    pix = 9 * W + 40
    s = pc.split32_np(emu["c2"].numpy()).copy()
    halves = s.view(np.float16).reshape(P, 2, 64)
    halves[pix, 1] = np.concatenate([halves[pix, 1, 32:], halves[pix, 1, :32]])
    got = torch.from_numpy(pc.split32_inverse_np(s))
    rep = check(emu, "corr2", c2=got)
    assert not rep.ok and set(rep.pixels.tolist()) == {pix} and set(rep.channels) <= set(range(32, 64)) and rep.only_tile() == (2, 1)
    ref = ref64(emu, "c2")
    old_pass = rel_l1(got, emu["c2"]) < 1e-6 and rel_l1(got, ref) < 2e-6
    assert old_pass == OLD_CRITERIA_PASS["split32_hi_lo_swapped"], (rel_l1(got, emu["c2"]), rel_l1(got, ref))


def test_gru_blend_reading_the_updated_hidden_state(emu):
    """q, in place: at one tile's pixels the blend reads h after a neighbouring block has stored it (here: its own new value)."""
    m = tile_mask(*TILE)
    stale = through_split32((1 - emu["z"]) * emu["new"] + emu["z"] * torch.tanh(emu["pre_q"]))
    got = torch.where(m[:, None], stale, emu["new"])
    rep = check(emu, "q", new=got)
    assert not rep.ok and rep.only_tile() == TILE
    old_pass = rel_l1(got, ref64(emu, "new")) < 1e-5
    assert old_pass == OLD_CRITERIA_PASS["gru_reads_updated_h"], rel_l1(got, ref64(emu, "new"))


def test_one_tap_plane_shifted_by_a_pixel(emu):
    """delta head: tap plane 4 of the second channel half is stored one pixel late."""
    got = emu["T"].clone()
    got[1:, 13] = emu["T"][:-1, 13]
    rep = check(emu, "delta", T=got)
    assert not rep.ok and set(rep.channels) == {13} and len(rep.tiles) > 1
    assert check(emu, "delta_sum", T=got, disp_new=emu["disp_new"]).n_fail > 0           # ... and the sum no longer belongs to these planes
    planes = F.pad(got.t().reshape(2, 9, H, W), (1, 1, 1, 1))
    s = sum(planes[:, tap, tap // 3:tap // 3 + H, tap % 3:tap % 3 + W].sum(0) for tap in range(9)).reshape(-1)
    delta_bad, delta = 0.01 * (s + emu["b_d2"]), emu["disp_new"] - emu["disp"]
    old_pass = rel_l1(delta_bad, delta) < 1e-5
    assert old_pass == OLD_CRITERIA_PASS["tap_plane_shifted"], rel_l1(delta_bad, delta)


def test_collapsed_window_ignoring_the_zero_padding_at_the_bottom_rim(emu):
    """z|r: the interior tile at ty0 = 8 evaluates its 9 x 9 disparity windows on a disparity that continues below the image instead of
    the unfold's zeros."""
    feat_bad = disp_features32(emu["disp"], pad_bottom_replicate=True)
    pre = conv32(torch.cat([emu["h"], feat_bad, emu["c2"]], 1), emu["w_zr"]) + emu["hzr"]
    m = tile_mask(*TILE)
    z = torch.where(m[:, None], torch.sigmoid(pre[:, :64]), emu["z"])
    rh = torch.where(m[:, None], through_split32(torch.sigmoid(pre[:, 64:]) * emu["h"]), emu["rh"])
    rz, rr = check(emu, "zr", z=z, rh=rh)
    assert not rz.ok and rz.only_tile() == TILE and set(rz.rows) <= {9, 10, 11}          # (row 8's windows end at row 12: inside)
    assert not rr.ok and rr.only_tile() == TILE
    old_pass = (rel_l1(z, ref64(emu, "z")) < 2e-6 and rel_l1(rh, ref64(emu, "rh")) < 2e-6
                and float((z - ref64(emu, "z")).abs().max()) < 5e-6 * float(ref64(emu, "z").abs().max()))
    assert old_pass == OLD_CRITERIA_PASS["collapsed_window_ignores_bottom_padding"], rel_l1(z, ref64(emu, "z"))


# ------------------------------------------------------------------------------------------------ the cost-volume walk
WALK_ALL = [(g, s, h, w, V, D) for g in cases.WALK_GEOMS for s in (0, 1) for h, w in cases.WALK_SHAPES for V in cases.WALK_VS for D in cases.WALK_DS]


def test_walk_yardstick_is_finite_and_positive_for_every_case():
    """The GPU test allows the kernel 4 x the fp32 oracle's own deviation from float64: a yardstick of 0 would reject everything, an
    infinite one nothing.  Also: Z stays positive over every hypothesis range (the geometries where it does not stay out)."""
    worst = {}
    for geom, stage, h, w, V, D in WALK_ALL:
        R = cases.walk_reference(geom, stage, h, w, V, D)
        for key in ("views", "fold"):
            ymax, yp = R["yardstick"][key]
            assert np.isfinite(ymax) and 0.0 < yp <= ymax < 1e-2, (geom, stage, h, w, V, D, key, ymax, yp)
            worst[key] = max(worst.get(key, 0.0), ymax)
        c = cases.walk_case(geom, stage, h, w, V)
        hyp = torch.tensor([-(D // 2) * c["incre"], 0.0, (D - 1 - D // 2) * c["incre"]]).view(3, 1, 1) + R["origin"].view(1, h, w)
        y, x = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        for m in c["Pij"]:
            assert float((m[2, 0] * x + m[2, 1] * y + m[2, 2] + m[2, 3] * hyp).min()) > 0.5
    print("  fp32 oracle against float64, max |err| / norm over all cases:", worst)


def test_walk_sample_one_texel_off():
    """One hypothesis of one pixel sampled one texel to the right: the per-element check names the pixel; the kernel-against-kernel
    criterion of test_cost_lines_matches_walk (4e-6 max(|vol|, 1)) is stated next to it."""
    from oracle import cer_oracle as O
    geom, stage, h, w, V, D = "lateral", 0, 19, 45, 1, 64
    c = cases.walk_case(geom, stage, h, w, V)
    R = cases.walk_reference(geom, stage, h, w, V, D)
    clean = O.cost_volume(c["fmaps"], c["poses"], c["intr"], D, c["incre"], c["disp_in"], c["shift"])[0][0].double()       # [P, D]
    ref, norm = R["fold"]
    ymax, _ = R["yardstick"]["fold"]
    assert pc.check_elementwise(clean, ref, norm, 4 * ymax, 0.0, "clean", h=h, w=w, tile=(1, 4)).ok
    shifted = c["Pij"].clone()
    shifted[0, 0, 2] += 1.0                                  # every sample one texel to the right ...
    off, _, _ = pc.cost_volume_ref64(c["fmaps"], shifted, D, c["incre"], c["disp_in"], c["shift"])
    pix, k = 7 * w + 21, 37
    got = clean.clone()
    got[pix, k] = off[0, pix, k]                             # ... taken for one hypothesis of one pixel
    rep = pc.check_elementwise(got, ref, norm, 4 * ymax, 0.0, "texel off", h=h, w=w, tile=(1, 4))
    assert rep.n_fail == 1 and rep.worst == (7, 21, k) and rep.only_row() == 7
    old_pass = float((got - clean).abs().max()) <= 4e-6 * max(float(clean.abs().max()), 1.0)
    assert old_pass == OLD_CRITERIA_PASS["walk_sample_one_texel_off"], float((got - clean).abs().max())


# ------------------------------------------------------------------------------------------------ the split32 layout in numpy
def test_split32_restatement_matches_the_documented_layout():
    """include/cer_mvs.h: per pixel and 32-channel chunk, 32 hi halves then 32 lo halves, x = hi + 2^-11 lo; hx_split clamps to +-65504."""
    f16 = lambda v: np.float16(v)
    x = np.zeros((2, 64), dtype=np.float32)
    x[0, 0] = 1.5                                            # an exact f16: lo = 0
    x[0, 1] = 1.0 + 2.0 ** -12                               # hi = 1, residual 2^-12 -> lo = 2^-1
    x[0, 2] = 3.0e-6                                         # below the f16 normal range (2^-14): hi is a subnormal multiple of 2^-24
    x[0, 3], x[0, 4], x[0, 5], x[0, 6] = 65504.0, -65504.0, 1.0e6, -3.0e38
    x[0, 7] = -0.0
    x[0, 33] = 0.1                                           # second chunk of pixel 0
    x[1, 31] = -2.75                                         # last channel of the first chunk of pixel 1
    s = pc.split32_np(x)
    assert s.shape == (2, 64) and s.dtype == np.float32
    hv = s.view(np.float16).reshape(2, 2, 2, 32)             # [pixel, chunk, hi | lo, channel in chunk]
    hi, lo = hv[:, :, 0], hv[:, :, 1]
    assert hi[0, 0, 0] == f16(1.5) and lo[0, 0, 0] == 0
    assert hi[0, 0, 1] == f16(1.0) and lo[0, 0, 1] == f16(0.5)
    h2 = np.float32(np.round(3.0e-6 / 2.0 ** -24) * 2.0 ** -24)
    assert np.float32(hi[0, 0, 2]) == h2 and lo[0, 0, 2] == f16((np.float32(3.0e-6) - h2) * np.float32(2048.0))
    assert hi[0, 0, 3] == f16(65504.0) and hi[0, 0, 4] == f16(-65504.0) and lo[0, 0, 3] == 0 and lo[0, 0, 4] == 0
    assert hi[0, 0, 5] == f16(65504.0) and hi[0, 0, 6] == f16(-65504.0) and lo[0, 0, 5] == 0 and lo[0, 0, 6] == 0      # saturation, never inf
    assert hi[0, 0, 7] == 0 and np.signbit(hi[0, 0, 7]) and lo[0, 0, 7] == 0 and not np.signbit(lo[0, 0, 7])          # -0 keeps its sign in hi
    assert hi[0, 1, 1] == f16(0.1) and hi[1, 0, 31] == f16(-2.75) and lo[1, 0, 31] == 0
    assert np.count_nonzero(s.view(np.float16)) == 1 + 2 + 2 + 4 + 2 + 1            # nothing else was written anywhere
    back = pc.split32_inverse_np(s)
    want = np.clip(x, -65504.0, 65504.0)
    assert np.all(np.abs(back - want) <= 2.0 ** -22 * np.abs(want) + 2.0 ** -35)
    assert back[0, 0] == 1.5 and back[0, 1] == x[0, 1] and back[0, 5] == 65504.0 and back[0, 7] == 0.0
    # the quantum the GPU module allows a split32 output, on values across the whole range
    r = (hashed((64, 64), 4300).numpy() * np.logspace(-9, 4.5, 64 * 64, dtype=np.float32).reshape(64, 64)).astype(np.float32)
    rt = pc.split32_inverse_np(pc.split32_np(r)).astype(np.float64)
    assert np.all(np.abs(rt - r) <= pc.split32_quantum(torch.from_numpy(r.astype(np.float64))).numpy())


def test_delta_tail_depth_is_the_kernels():
    assert pc.delta_tail_depth(256) == 20 and pc.delta_tail_depth(512) == 32
    (ref, mag, a), (dref, dmag, da) = pc.delta_tail_ref64(torch.ones(4, 256, dtype=torch.float64), torch.full((9, 256), 0.5), 1.0,
                                                          torch.full((4,), 2.0, dtype=torch.float64), 2, 2)
    c01 = float(np.float32(0.01))
    assert torch.allclose(dref, torch.full((4,), c01 * (4 * 128.0 + 1.0), dtype=torch.float64))       # 2 x 2 image: every pixel a corner, 4 taps of 9 inside
    assert torch.allclose(ref, dref + 2.0) and torch.equal(mag, dmag + 2.0) and torch.equal(a, da)
