"""The element-wise checker of tests/parity_check.py on planted corruptions of a 296 x 400 x 64 reference (the bench's feature map):
each corruption is of a COPY OF THE REFERENCE, no kernel is involved.  For the stale tile and the wrong last row the global metric the
end-to-end tests assert (rel_l1 < 1e-4) stays below its bar - the blind spot, written down as a fact - while the
checker fails and names the tile / the row.  Also pins the float64 cost-volume restatement to the oracle.  CPU only."""
import pytest
import torch

from conftest import rel_l1
from parity_check import (assert_covered, assert_elementwise, check_elementwise, cost_subset, cost_volume_ref64, partial_tile_mask, poison_f16,
                          poison_f32, rim_mask, seam_mask)
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
