"""Element-wise parity of one GRU iteration's kernels AT RAGGED SIZES WITH EVERY TILE HEIGHT (run on the GPU box: pytest -m gpu).

tests/test_fullsize_parity_gpu.py holds every output element of the s16 update loop to a float64 bound, but only with the production
tile choice at shapes whose widths are multiples of 16 and whose heights are multiples of most tile heights: the picker reaches 6 of the
13 kernel families of ``cer_conv3x3_s16`` there, and none of them with a partial tile column.  tests/test_conv_s16_gpu.py forces the tile
height at ragged sizes but judges a global mean, which one wrong tile, last row or rim pixel passes (tests/test_parity_check_cpu.py).
Here the same check (``check_iteration`` of tests/s16_iteration_check.py: both hoisted convolutions, both lookup forms, corr2, z|r with the
collapsed disparity source and the rim correction, q / GRU in place with r*h in c1's buffer, the delta head with both stages' weights,
delta_sum; NaN sentinels in every output and in the inputs' padding slots; the bounds and constants of the full-size module, none
replaced, none fitted) runs with ``ops.TILE_MT`` forced to 2, 3 and 4 in all three arithmetic forms at the smallest shapes at which each
tiling edge exists:

  37 x 33   for every tile height 4 / 8 / 12 / 16 at least one interior tile (16 rows: rows 16..31, columns 16..31, the only one), border
            tiles, the rim-first block order, a partial last tile row (5 rows of 16, 1 row of 12) and a one-pixel last tile column
  33 x 37   a last tile row of exactly one image row for 4 / 8 / 16-row tiles, a 5-pixel last column
  17 x 48   width a multiple of 16, h = TH + 1 for 16-row tiles
  13 x 37, 9 x 21, 5 x 70    images shorter than the tall tiles: one clamped tile row, several tile columns, 131 of 320 padding slots at 9 x 21
  1 x 40, 40 x 2, 2 x 3      a pixel lies on several image edges at once: the rim correction's corner taps

A forced height is honoured only where the family exists (2 / 4 for 128 / 256 output channels, 2 .. 3 for 64 channels in the fp8 / FP6
forms, 2 .. 4 in the f16x3-terms form); elsewhere the picker decides, and on images this small it returns MT = 2 (asserted: that is why the
forcing is needed).  Each case asserts the tile height of each launch through the restated dispatch; the last test asserts over everything
that ran that each of the 13 families ran each of its epilogues (64: LINEAR, RELU, GRU; 128: LINEAR, GATES; 256: DELTA) with a partial
last tile in x, a partial last tile in y, a one-row last tile and an image shorter than the tile, z|r and q with interior and with border
tiles.  tests/test_s16_ragged_cpu.py proves the same census from the dispatch alone.

Measured on an MI355X (profiles/s16_ragged_parity.json, written only under CER_PARITY_RECORD=1 by a whole-module run; a plain run writes
nothing): worst max (99.9th-percentile) |err| / bound over all shapes and tile heights, f16x3 terms / fp8 / FP6 - corr2 0.30 (0.14) / 0.29
(0.19) / 0.24 (0.17), hoisted z|r 0.20 / 0.16 / 0.10, hoisted q 0.18 / 0.13 / 0.10, q / GRU 0.066 / 0.063 / 0.048, z 0.038 / 0.023 / 0.015, r*h
0.031 / 0.019 / 0.015, delta head <= 0.008, delta_sum <= 0.062; lookup D = 64 0.10, D = 44 0.16, delta form 0.084 (disparity) and 0.11 (features).
Nothing turned red: no kernel was changed.  81 cases + 2 in 3.3 s of module wall time (5.4 s with start-up); the slowest case 0.43 s (the first:
it builds the model), the others <= 0.16 s."""
import json
import os
import time

import pytest
import torch

from conftest import REPO
from s16_iteration_check import (FORMS, RAGGED_CASES, RAGGED_SHAPES, census, census_gaps, check_iteration, expected_tile_height, s16_grid)

pytestmark = pytest.mark.gpu

WORST = {}               # {"kernel/form": [worst max ratio, worst p99.9 ratio]} over shapes and tile heights
RAN = {}                 # {(h, w, form, tile_mt): launches} of the cases that passed


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _module_setup(dev):
    from cer_mvs_amd import ops
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    t0 = time.time()
    yield
    torch.set_num_threads(n)
    ops.check_overflow(dev)                            # (NaN sentinels in padding slots may have raised the sticky saturation flag)
    target = os.environ.get("CER_PARITY_RECORD", "")
    if target and set(RAN) == set(RAGGED_CASES):       # a whole-module run only
        path = os.path.join(REPO, "profiles", "s16_ragged_parity.json") if target == "1" else target
        out = {"worst_ratio_to_bound": {k: {"max": v[0], "p999": v[1]} for k, v in sorted(WORST.items())}, "cases": len(RAN),
               "module_wall_s": round(time.time() - t0, 1)}
        with open(path, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)


@pytest.fixture
def tile_mt():
    from cer_mvs_amd import ops
    yield ops
    ops.TILE_MT = 0


def test_unforced_picker_takes_the_short_tiles_everywhere(dev):
    """Without forcing, every launch at these shapes gets MT = 2 (4-row tiles for 128 / 256 output channels, 8-row tiles for 64): the
    other families are reached only by forcing."""
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    for h, w in RAGGED_SHAPES:
        for form in FORMS:
            for cout in (64, 128, 256):
                assert s16_grid(h, w, cout, form, ncu, 0)[1] == (8 if cout == 64 else 4), (h, w, form, cout)


@pytest.mark.parametrize("h,w,form,mt", RAGGED_CASES, ids=[f"{h}x{w}-{f}-mt{m}" for h, w, f, m in RAGGED_CASES])
def test_gru_iteration_ragged(dev, tile_mt, h, w, form, mt):
    tile_mt.TILE_MT = mt
    rec = {}
    launches = check_iteration(dev, h, w, form, tile_mt=mt, record=rec)
    for name, cout, epi, dsrc, th, blocks in launches:                               # which tile height ran, stated without the picker
        assert th == expected_tile_height(cout, form, mt), (name, th)
        assert blocks == -(-h // th) * -(-w // 16) * (cout // (64 if cout == 64 else 128)), (name, blocks)
    for key, fig in rec["kernels"].items():
        k = f"{key.split('/')[2]}/{form}"
        worst = WORST.setdefault(k, [0.0, 0.0])
        worst[0], worst[1] = max(worst[0], fig["max_ratio_to_bound"]), max(worst[1], fig["p999_ratio_to_bound"])
    RAN[(h, w, form, mt)] = launches


def test_census_of_what_ran():
    """Over the whole parametrisation: each of the 13 families ran each of its epilogues at every edge.  Counts only cases that passed,
    so it needs the whole module (it runs last)."""
    missing = [c for c in RAGGED_CASES if c not in RAN]
    assert not missing, f"{len(missing)} of {len(RAGGED_CASES)} cases did not run or did not pass, the first: {missing[0]}"
    seen = census((h, w, form, launches) for (h, w, form, _), launches in RAN.items())
    assert len(seen) == 39 and census_gaps(seen) == []             # 6 families x (LINEAR, GATES, DELTA) + 7 x (LINEAR, RELU, GRU)
    assert all("rim_first" in seen[k] for k in seen if k[1] in ("GATES", "GRU"))      # both block orders of the disparity launches ran
    assert all(v[0] <= 1.0 for v in WORST.values())
