"""The element-wise checker of tests/parity_check.py on planted corruptions of a 296 x 400 x 64 reference (the bench's feature map):
each corruption is of a COPY OF THE REFERENCE, no kernel is involved.  For the stale tile and the wrong last row the global metric the
end-to-end tests assert (rel_l1 < 1e-4) stays below its bar - the blind spot, written down as a fact - while the
checker fails and names the tile / the row.  Also pins the float64 cost-volume restatement to the oracle.  The same at the encoder
kernels' geometries (2 x 32 tiles of a stride-2 output, per-tile statistics records; bar rel_l1 < 1e-5), and the chained float64 encoder
reference of tests/test_encoder_parity_gpu.py against the oracle.  CPU only."""
import pytest
import torch

from conftest import rel_l1
from parity_check import (ENC_TILE_S2, assert_covered, assert_elementwise, check_batch, check_elementwise, check_stats_records, cost_subset,
                          cost_volume_ref64, enc_chain_ref64, partial_tile_mask, poison_f16, poison_f32, rim_mask, seam_mask,
                          stats_records_ref64)
from test_oracle_golden import hashed

H, W, C = 296, 400, 64
TILE = (8, 16)
C_FP32 = 1e-6            # the per-element constant of tests/test_conv_s16_gpu.py::test_conv_s16_two_sources_and_error_bound


@pytest.fixture(scope="module")
def ref():
    """(reference [P, 64] in float64, its magnitude, the 'previous iteration': the reference moved by a smooth 5 % perturbation)."""
    r = hashed((H * W, C), 4101, -1.0, 1.0).double()
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    smooth = 0.05 * torch.sin(0.021 * x + 0.4) * torch.cos(0.033 * y - 0.2)
    prev = r * (1.0 + smooth.reshape(-1, 1))
    return r, r.abs() + 1.0, prev


def img(t):
    return t.view(H, W, C)


def test_clean_copy_passes(ref):
    r, mag, _ = ref
    got = r.float()                     # an fp32 rounding of the reference: 6e-8 relative
    rep = assert_elementwise(got, r, mag, C_FP32, where="clean", h=H, w=W, tile=TILE)
    assert rep.ok and rep.n == H * W * C and rep.max_ratio < 0.1


def test_stale_tile_is_invisible_to_rel_l1_and_named_by_the_checker(ref):
    """(a) one 8 x 16 tile holds the previous iteration's values: 1.1e-3 of the pixels x <= 5 %."""
    r, mag, prev = ref
    ty, tx = 17, 9
    got = r.clone()
    img(got)[ty * 8:ty * 8 + 8, tx * 16:tx * 16 + 16] = img(prev)[ty * 8:ty * 8 + 8, tx * 16:tx * 16 + 16]
    assert 0 < rel_l1(got, r) < 1e-4                     # the end-to-end bar does not see it
    rep = check_elementwise(got, r, mag, C_FP32, where="stale tile", h=H, w=W, tile=TILE)
    assert not rep.ok and rep.only_tile() == (ty, tx)
    assert set(rep.rows) <= set(range(ty * 8, ty * 8 + 8)) and set(rep.cols) <= set(range(tx * 16, tx * 16 + 16))
    with pytest.raises(AssertionError, match=r"confined to tile \(17, 9\)"):
        assert_elementwise(got, r, mag, C_FP32, where="stale tile", h=H, w=W, tile=TILE)


def test_wrong_last_row_is_invisible_to_rel_l1_and_named_by_the_checker(ref):
    """(b) the last image row 1 % off: 1 / 296 of the pixels x 1 %."""
    r, mag, _ = ref
    got = r.clone()
    img(got)[H - 1] *= 1.01
    assert 0 < rel_l1(got, r) < 1e-4
    rep = check_elementwise(got, r, mag, C_FP32, where="last row", h=H, w=W, tile=TILE)
    assert not rep.ok and rep.only_row() == H - 1 and rep.on_rim == rep.n_fail
    assert set(ty for ty, _ in rep.tiles) == {(H - 1) // 8}
    with pytest.raises(AssertionError, match=r"confined to image row 295 \(the last row\)"):
        assert_elementwise(got, r, mag, C_FP32, where="last row", h=H, w=W, tile=TILE)


def test_swapped_tiles_are_named(ref):
    """(c) one tile swapped with its right neighbour (a wrong block -> tile mapping)."""
    r, mag, _ = ref
    ty, tx = 36, 23                                      # the last tile row
    got = r.clone()
    a = img(r)[ty * 8:ty * 8 + 8, tx * 16:tx * 16 + 16].clone()
    b = img(r)[ty * 8:ty * 8 + 8, (tx + 1) * 16:(tx + 1) * 16 + 16].clone()
    img(got)[ty * 8:ty * 8 + 8, tx * 16:tx * 16 + 16] = b
    img(got)[ty * 8:ty * 8 + 8, (tx + 1) * 16:(tx + 1) * 16 + 16] = a
    rep = check_elementwise(got, r, mag, C_FP32, where="swap", h=H, w=W, tile=TILE)
    assert not rep.ok and set(rep.tiles) == {(ty, tx), (ty, tx + 1)} and rep.only_tile() is None
    assert "(36, 23)" in rep.message() and "(36, 24)" in rep.message()


def test_zeroed_channel_group_of_one_tile_is_named(ref):
    """(d) one 16-channel group of one tile zeroed (an n-tile of a block that never stored)."""
    r, mag, _ = ref
    ty, tx, g = 0, 24, 2                                 # top right corner tile, channels 32..47
    got = r.clone()
    img(got)[ty * 8:ty * 8 + 8, tx * 16:tx * 16 + 16, g * 16:g * 16 + 16] = 0.0
    rep = check_elementwise(got, r, mag, C_FP32, where="zeroed group", h=H, w=W, tile=TILE)
    assert not rep.ok and rep.only_tile() == (ty, tx) and set(rep.channels) <= set(range(32, 48)) and len(rep.channels) == 16
    assert rep.on_rim > 0 and "channels - " in rep.message()


def test_sentinels_and_masks():
    """A NaN left in the output fails the coverage check and is located; the f16 sentinel is a NaN in both halves of every slot."""
    h, w = 37, 400                                       # a row slab: the last tile row is partial (37 = 4 x 8 + 5)
    out = torch.zeros(h * w, 64)
    assert_covered(out, "clean", h, w)
    out.view(h, w, 64)[32:37, 16:32] = float("nan")
    with pytest.raises(AssertionError, match=r"confined to tile \(4, 1\)"):
        assert_covered(out, "skipped", h, w)
    rep = check_elementwise(out, torch.zeros_like(out), torch.ones_like(out), 1.0, h=h, w=w)
    assert rep.n_fail == 5 * 16 * 64 and rep.in_partial_tile == rep.n_fail
    t = poison_f16(torch.zeros(8, 4))
    assert torch.isnan(t.view(torch.float16)).all() and t.view(torch.float16).numel() == 64
    assert torch.isnan(poison_f32(torch.zeros(3))).all()
    assert int(rim_mask(5, 7).sum()) == 2 * 7 + 2 * 3 and int(partial_tile_mask(296, 400).sum()) == 0
    s = seam_mask(70, 70)
    assert s[31, 5] and s[32, 5] and s[5, 63] and s[5, 64] and not s[5, 5] and not s[0, 1] and not s[69, 1]
    # a subset checked by pixel id is located in the full image
    pix = torch.tensor([0, 399, 400 * 36 + 17])
    rep = check_elementwise(torch.tensor([0.0, 0.0, 1.0]), torch.zeros(3), torch.ones(3), 0.5, h=h, w=w, pixels=pix)
    assert rep.n_fail == 1 and rep.only_tile() == (4, 1) and rep.only_row() == 36


def test_cost_subset_holds_rim_seams_and_border_tiles():
    idx, must = cost_subset(H, W)
    chosen = torch.zeros(H * W, dtype=torch.bool)
    chosen[idx] = True
    assert bool(chosen[must.reshape(-1)].all()) and bool(chosen[rim_mask(H, W).reshape(-1)].all()) and bool(chosen[seam_mask(H, W).reshape(-1)].all())
    assert idx.numel() >= 0.08 * H * W
    interior = chosen & ~must.reshape(-1)
    assert 0.03 * H * W < int(interior.sum()) < 0.05 * H * W           # 5 % of the pixels the fixed part does not hold already


@pytest.mark.parametrize("D,N,shift", [(64, 64, True), (44, 320, False)])
def test_cost_volume_restatement_equals_the_oracle_in_float64(D, N, shift):
    """All pixels of a small case: the restatement and oracle.cer_oracle.cost_volume, both in float64, agree to 1e-12 - on a converging
    pair of the synthetic scene's kind, with samples that leave the source map on every side."""
    from cer_mvs_amd.synthetic import synthetic_scene
    from oracle import cer_oracle as O
    h, w, V = 13, 22, 3
    _, poses, intr, _ = synthetic_scene(4 * h, 4 * w, V, seed=0)
    poses, intr = poses[0].double(), intr[0].double()
    intr[:, :2] /= 4
    poses[2, 0, 3] += 900.0                              # one view pushed sideways: part of its samples fall outside
    fmaps = hashed((V + 1, 64, h, w), 4201, -2, 2).double()
    incre = 0.0025 / N
    disp_in = (torch.zeros(h, w) if shift else hashed((h, w), 4202, 0.0005, 0.002)).double()
    ref, origin_ref = O.cost_volume(fmaps, poses, intr, D, incre, disp_in, shift)
    assert ref.dtype == torch.float64
    Pij = O.pij_matrices(poses, intr, [0] * V, list(range(1, V + 1)))
    vol, norm, origin = cost_volume_ref64(fmaps, Pij, D, incre, disp_in, shift)
    assert torch.equal(origin.view(h, w), origin_ref.double())
    assert float((vol - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    assert float((ref == 0).double().mean()) > 0.01 and float(ref.abs().max()) > 0.1
    assert bool((norm >= vol.abs() - 1e-12).all())
    # and a subset is the same rows
    pix = torch.tensor([0, 5, w - 1, h * w - 1])
    sub, _, _ = cost_volume_ref64(fmaps, Pij, D, incre, disp_in, shift, pixels=pix)
    assert torch.equal(sub, vol[:, pix])


# ------------------------------------------------------------------------------------------------ encoder geometries
EN, EH, EW, EC = 40, 10, 67, 64          # a stride-2 3 x 3 output of the encoder parity module: 40 images of 10 x 67, 2 x 32 tiles
C_ENC = 2e-6                             # the three-term constant of tests/test_hip_parity.py::test_stem_on_matrix_cores


@pytest.fixture(scope="module")
def enc_ref():
    r = hashed((EN, EH, EW, EC), 4301, -1.0, 1.0).double()
    return r, r.abs() + 1.0


def test_encoder_wrong_stride2_tile_is_invisible_to_rel_l1_and_named(enc_ref):
    """One 2 x 32 tile of one image 1e-3 off (relative): 64 of 26 800 pixels - the whole-encoder bar rel_l1 < 1e-5 passes it."""
    r, mag = enc_ref
    n, ty, tx = 23, 3, 1
    got = r.clone()
    got[n, ty * 2:ty * 2 + 2, tx * 32:tx * 32 + 32] *= 1.001
    assert 0 < rel_l1(got, r) < 1e-5
    rep = check_elementwise(got[n].reshape(EH * EW, EC), r[n].reshape(EH * EW, EC), mag[n].reshape(EH * EW, EC), C_ENC, where="tile",
                            h=EH, w=EW, tile=ENC_TILE_S2)
    assert not rep.ok and rep.only_tile() == (ty, tx)
    with pytest.raises(AssertionError, match=r"(?s)image 23 of 40.*confined to tile \(3, 1\)"):
        check_batch(got, r, mag, C_ENC, where="tile", h=EH, w=EW, tile=ENC_TILE_S2)
    assert check_batch(r.float(), r, mag, C_ENC, where="clean", h=EH, w=EW, tile=ENC_TILE_S2)["max_ratio"] < 0.1


def test_encoder_wrong_last_row_is_invisible_to_rel_l1_and_named(enc_ref):
    """The last row of one image 1e-3 off: 67 of 26 800 pixels."""
    r, mag = enc_ref
    got = r.clone()
    got[EN - 1, EH - 1] *= 1.001
    assert 0 < rel_l1(got, r) < 1e-5
    with pytest.raises(AssertionError, match=r"(?s)image 39 of 40.*confined to image row 9 \(the last row\)"):
        check_batch(got, r, mag, C_ENC, where="row", h=EH, w=EW, tile=ENC_TILE_S2)


def test_swapped_statistics_records_are_invisible_to_the_reduce_and_named(enc_ref):
    """Two neighbouring tiles' (sum, sum of squares) records swapped - a record written under the wrong tile id: the per-image totals,
    hence the statistics and everything after them, do not change at all; the per-tile check names both tiles."""
    r, _ = enc_ref
    out = r.float()
    S, Q, _ = stats_records_ref64(out, ENC_TILE_S2)
    part = torch.stack([S, Q], -1).float()
    assert tuple(part.shape) == (EN, 5 * 3, EC, 2)
    ok, msg, mx = check_stats_records(part, out, ENC_TILE_S2, 19, "clean")
    assert ok and mx < 0.1, msg
    n, ty, tx = 7, 4, 1                                   # the last tile row; (4, 2) is the partial last tile
    bad = part.clone()
    a, b = ty * 3 + tx, ty * 3 + tx + 1
    bad[n, a], bad[n, b] = part[n, b], part[n, a]
    assert torch.equal(bad.double().sum(1), part.double().sum(1)) and rel_l1(bad.double().sum(1), part.double().sum(1)) < 1e-5
    ok, msg, _ = check_stats_records(bad, out, ENC_TILE_S2, 19, "swap")
    assert not ok and "(7, 4, 1), (7, 4, 2)" in msg and msg.count("(7,") == 2
    nan = part.clone()
    nan[3, 0, 5, 1] = float("nan")                        # a record nobody wrote keeps its sentinel
    ok, msg, _ = check_stats_records(nan, out, ENC_TILE_S2, 19, "sentinel")
    assert not ok and "(3, 0, 0)" in msg


@pytest.mark.parametrize("kind,which", [("instance", "fnet"), ("none", "cnet")])
def test_chained_encoder_reference_equals_the_oracle(kind, which):
    """enc_input_ref64 / enc_conv_ref64 chained through the whole HR encoder with float64 instance-norm statistics, in the schedule of
    the HIP engine (raw outputs + statistics, normalisation by the consumer, residual merges as two-tensor inputs) = the oracle's
    encoder, at 36 x 52 (9 x 13 feature pixels, odd sizes on the way)."""
    from cer_mvs_amd.synthetic import fill_state_dict, synthetic_scene
    from oracle import cer_oracle as O
    from test_oracle_golden import blank_state_dict
    sd = fill_state_dict(blank_state_dict(), seed=5)
    images, _, _, _ = synthetic_scene(36, 52, 1, seed=8)
    x = images[0].float() * (2 / 255.0) - 1
    ref = O.encoder(x, sd, which + ".", kind)
    outs = {}
    got = enc_chain_ref64(x, sd, which + ".", kind, outputs=outs)
    assert got.shape == ref.shape and len(outs) == 10
    assert rel_l1(got, ref) < 1e-6
    ref64 = O.encoder(x.double(), {k: v.double() for k, v in sd.items()}, which + ".", kind)
    assert rel_l1(got, ref64) < 1e-12
