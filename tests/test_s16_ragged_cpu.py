"""CPU companion of tests/test_s16_ragged_parity_gpu.py: what that module claims about its own cases, proved without a GPU from the
restated dispatch of tests/s16_iteration_check.py - the census (every one of the 13 kernel families of ``cer_conv3x3_s16`` x its epilogues
meets a partial last tile in x and in y, a one-row last tile, an image shorter than the tile, z|r and q also interior and border tiles),
the reason for forcing (the picker alone returns MT = 2 at every ragged shape), the restated dispatch against what the full-size module
recorded with ``tile_mt = 0``, the checker on errors planted into a float64 convolution at 37 x 33 that the global mean of
tests/test_conv_s16_gpu.py passes, and the placement of the lookup's planted indices."""
import json
import os

import pytest
import torch

from conftest import REPO, rel_l1
from parity_check import check_elementwise, conv_ref
from s16_iteration_check import (C_CONV, CASES, EDGES, EDGES_DISP, FAMILIES, FORMS, RAGGED_CASES, RAGGED_SHAPES, RAGGED_TILE_MT, census,
                                 census_gaps, expected_tile_height, family, family_epilogues, iteration_launches, launch_edges,
                                 planted_indices, s16_grid)
from test_oracle_golden import hashed

NCU = 256                # compute units of an MI355X

# (blocks, tile height) per output-channel count of the full-size cases at 256 CUs with tile_mt = 0, as the dispatch was restated when
# profiles/fullsize_parity.json was recorded (its "grids" hold the same block counts)
FULLSIZE_GRIDS = {
    (296, 400, "f16x3terms"): {64: (475, 16), 128: (925, 8), 256: (1850, 8)},
    (296, 400, "fp8corr"): {64: (925, 8), 128: (925, 8), 256: (1850, 8)},
    (296, 400, "fp6corr"): {64: (925, 8), 128: (925, 8), 256: (1850, 8)},
    (384, 512, "fp8corr"): {64: (1024, 12), 128: (1536, 8), 256: (3072, 8)},
    (540, 960, "fp8corr"): {64: (2700, 12), 128: (4080, 8), 256: (8160, 8)},
    (37, 400, "fp8corr"): {64: (125, 8), 128: (250, 4), 256: (500, 4)},
    (51, 400, "fp8corr"): {64: (175, 8), 128: (325, 4), 256: (350, 8)},
}


def ragged_runs(cases=RAGGED_CASES):
    return [(h, w, form, iteration_launches(h, w, form, NCU, mt)) for h, w, form, mt in cases]


def test_case_list():
    assert len(RAGGED_CASES) == len(set(RAGGED_CASES)) == len(RAGGED_SHAPES) * 3 * 3 == 81
    assert set(RAGGED_TILE_MT) == {2, 3, 4} and set(FORMS) == {"f16x3terms", "fp8corr", "fp6corr"}
    assert len(FAMILIES) == len(set(FAMILIES)) == 13
    assert max(h * w for h, w in RAGGED_SHAPES) <= 37 * 48           # seconds, not the workload's sizes


def test_census_every_family_and_epilogue_meets_every_edge():
    seen = census(ragged_runs())
    assert census_gaps(seen) == []
    assert set(seen) == {(fam, epi) for fam in FAMILIES for epi in family_epilogues(fam)} and len(seen) == 39
    for (fam, epi), edges in seen.items():
        assert set(EDGES) <= edges, (fam, epi)
        if epi in ("GATES", "GRU"):
            assert set(EDGES_DISP) | {"rim_first"} <= edges, (fam, epi)
    # and the census notices a hole: without the two tallest shapes q has no interior 12- or 16-row tile, without forcing 7 families never run
    gaps = census_gaps(census(ragged_runs([c for c in RAGGED_CASES if c[:2] not in ((37, 33), (33, 37))])))
    assert {(fam, epi) for fam, epi, miss in gaps if "interior" in miss} == {((2, 2, 3, f8), "GRU") for f8 in range(3)} | {((2, 2, 4, 0), "GRU")}
    unforced = census((h, w, form, iteration_launches(h, w, form, NCU, 0)) for h, w in RAGGED_SHAPES for form in FORMS)
    assert {fam for fam, _ in unforced} == {(1, 4, 2, f8) for f8 in range(3)} | {(2, 2, 2, f8) for f8 in range(3)}


def test_edges_of_the_shapes_as_documented():
    """The table of the GPU module's docstring, shape by shape."""
    e = lambda h, w, th: launch_edges(h, w, th, True)
    for th in (4, 8, 12, 16):
        assert {"interior", "border", "rim_first", "partial_x", "partial_y"} <= e(37, 33, th), th
    assert 37 % 16 == 5 and 37 % 12 == 1 and 33 % 16 == 1 and "one_row" in e(37, 33, 12)
    for th in (4, 8, 16):
        assert "one_row" in e(33, 37, th) and 37 % 16 == 5
    assert "one_row" not in e(33, 37, 12)
    assert "one_row" in e(17, 48, 16) and "partial_x" not in e(17, 48, 16)
    for h, w in ((13, 37), (9, 21), (5, 70)):
        assert "short" in e(h, w, 16) and "interior" not in e(h, w, 16) and -(-w // 16) >= 2
    assert 5 * 2 * 32 - 9 * 21 == 131                                 # padding slots of the 9 x 21 image (2-row x 16-column m-tiles)
    for h, w in ((1, 40), (40, 2), (2, 3)):
        assert min(h, w) <= 2 and e(h, w, 4) >= {"border"} and "interior" not in e(h, w, 4)


def test_forcing_is_needed_and_honoured_only_where_valid():
    for h, w in RAGGED_SHAPES:
        for form in FORMS:
            for cout in (64, 128, 256):
                assert s16_grid(h, w, cout, form, NCU, 0)[1] == (8 if cout == 64 else 4), (h, w, form, cout)
                for mt in (1, 2, 3, 4, 5):
                    blocks, th = s16_grid(h, w, cout, form, NCU, mt)
                    assert th == expected_tile_height(cout, form, mt), (h, w, form, cout, mt)
                    assert blocks == -(-h // th) * -(-w // 16) * (1 if cout == 64 else cout // 128)
    assert family(64, "f16x3terms", 16) == (2, 2, 4, 0) and family(256, "fp6corr", 8) == (1, 4, 4, 2) and family(128, "fp8corr", 4) == (1, 4, 2, 1)
    # a forced height is honoured at the full-size shapes too (where the picker would choose otherwise)
    assert s16_grid(296, 400, 64, "f16x3terms", NCU, 3) == (25 * 25, 12) and s16_grid(296, 400, 64, "fp8corr", NCU, 4) == (925, 8)
    assert s16_grid(296, 400, 128, "fp8corr", NCU, 3) == (925, 8) and s16_grid(296, 400, 128, "fp8corr", NCU, 2) == (74 * 25, 4)


def test_restated_dispatch_unforced_equals_the_recorded_grids():
    assert set(FULLSIZE_GRIDS) == set(CASES)
    with open(os.path.join(REPO, "profiles", "fullsize_parity.json")) as f:
        recorded = json.load(f)["grids"]
    for (h, w, form), grids in FULLSIZE_GRIDS.items():
        for cout, want in grids.items():
            assert s16_grid(h, w, cout, form, NCU) == s16_grid(h, w, cout, form, NCU, 0) == want, (h, w, form, cout)
            assert recorded[f"{h}x{w}/{form}"][str(cout)] == want[0]


# ------------------------------------------------------------------------------------------------ planted errors at 37 x 33
H, W = 37, 33


@pytest.fixture(scope="module")
def conv37x33():
    """A float64 3 x 3 convolution 64 -> 64 at 37 x 33 and the magnitude its bound is made of."""
    x = hashed((H * W, 64), 7301, -1.0, 1.0).double()
    wt = hashed((64, 64, 3, 3), 7302, -0.1, 0.1)
    b = hashed((64,), 7303, -0.1, 0.1)
    return conv_ref(x, x.abs(), wt, b, H, W)


# (tile height, (tile_y, tile_x), relative error): the last tile of the 16-row tiling (rows 32..36 x column 32: 5 pixels), the one-row
# last tile of the 12-row tiling, the partial last tile row of the 8-row tiling, the one-pixel corner tile of the 4-row tiling
PLANTED_TILES = [(16, (2, 2), 1e-4), (12, (3, 0), 5e-5), (8, (4, 1), 1e-5), (4, (9, 2), 1e-3)]


@pytest.mark.parametrize("widen", [1.0, 30.0, 45.0], ids=list(FORMS))
@pytest.mark.parametrize("th,tile,rel", PLANTED_TILES, ids=[f"th{t[0]}" for t in PLANTED_TILES])
def test_one_wrong_tile_passes_the_mean_and_is_named(conv37x33, th, tile, rel, widen):
    ref, mag = conv37x33
    got = ref.clone()
    ty, tx = tile
    got.view(H, W, 64)[ty * th:(ty + 1) * th, tx * 16:(tx + 1) * 16] *= 1.0 + rel * widen
    assert 0 < rel_l1(got, ref) < 1e-6 * widen                        # the bar of tests/test_conv_s16_gpu.py does not see it
    rep = check_elementwise(got, ref, mag, C_CONV * widen, where="tile", h=H, w=W, tile=(th, 16))
    assert not rep.ok and rep.only_tile() == tile and rep.in_partial_tile == rep.n_fail
    assert f"{th} x 16 tile ({ty}, {tx})" in rep.message() and f"confined to tile ({ty}, {tx})" in rep.message()
    if th != 8:                                                       # reported by another launch's tile, the name would be wrong
        assert check_elementwise(got, ref, mag, C_CONV * widen, where="tile", h=H, w=W, tile=(8, 16)).only_tile() != tile


@pytest.mark.parametrize("widen", [1.0, 30.0, 45.0], ids=list(FORMS))
@pytest.mark.parametrize("row", [36, 32, 16])
def test_one_wrong_row_passes_the_mean_and_is_named(conv37x33, row, widen):
    """The last image row (the one-row tile of the 12-row tiling), the first row of the last 16-row and 8-row tile, the first row of the
    interior 16-row tile."""
    ref, mag = conv37x33
    got = ref.clone()
    got.view(H, W, 64)[row] *= 1.0 + 2e-5 * widen
    assert 0 < rel_l1(got, ref) < 1e-6 * widen
    rep = check_elementwise(got, ref, mag, C_CONV * widen, where="row", h=H, w=W, tile=(16, 16))
    assert not rep.ok and rep.only_row() == row and set(ty for ty, _ in rep.tiles) == {row // 16}
    assert f"confined to image row {row}" + (" (the last row)" if row == H - 1 else "") in rep.message()
    assert check_elementwise(ref.float(), ref, mag, C_CONV * widen, where="clean", h=H, w=W, tile=(16, 16)).ok


# ------------------------------------------------------------------------------------------------ planted lookup indices
def old_planting(P):
    """The full-size module's statements before the k % P placement, on a vector of marks."""
    steps = torch.zeros(P)
    steps[::97] = 7.0
    steps[0], steps[1], steps[2], steps[3], steps[P - 1], steps[P - 2] = -100.0, 1e6, 3.0, -22.0, 1e6, -100.0
    return steps


@pytest.mark.parametrize("P", [98, 99, 189, 194, 195, 37 * 33, 37 * 400, 51 * 400, 296 * 400, 384 * 512, 540 * 960])
def test_planted_indices_are_where_they_were(P):
    integral, planted = planted_indices(P)
    assert integral == list(range(0, P, 97)) and [k for k, _ in planted] == [0, 1, 2, 3, P - 1, P - 2]
    steps = torch.zeros(P)
    steps[integral] = 7.0
    for k, v in planted:
        steps[k] = v
    assert torch.equal(steps, old_planting(P))


@pytest.mark.parametrize("P", [1, 2, 3, 5, 6])
def test_planted_indices_fit_tiny_images(P):
    integral, planted = planted_indices(P)
    assert integral == [0] and all(0 <= k < P for k, _ in planted) and [v for _, v in planted] == [-100.0, 1e6, 3.0, -22.0, 1e6, -100.0]
    if P >= 6:
        assert sorted(k for k, _ in planted) == [0, 1, 2, 3, P - 2, P - 1]
