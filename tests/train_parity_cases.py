"""The inputs of tests/test_train_parity_gpu.py and their edge census, shared with tests/test_train_parity_cpu.py, which checks the census
without a GPU: what each case is built from, what it must exercise, and the counts that prove it does.  Inputs are `hashed(...)`:
deterministic, the same on every machine."""
import torch

from parity_check import tl_coord32, upsample_ranges_brute
from test_oracle_golden import hashed

CORR_GEOM = dict(B=2, N=3, H1=9, W1=13, H2=11, W2=7)         # 117 = 7 * 16 + 5 pixels, 77 = 4 * 16 + 13 texels per view
CORR_CASES = [(64, 0), (64, 1), (64, 2), (128, 1), (192, 1), (256, 1)]      # (C, radius)
LOOKUP_CASES = [(45, 3, 5, 273), (23, 4, 2, 64), (128, 4, 7, 130), (2, 1, 0, 65), (64, 3, 5, 273)]      # (D, L, r, P)
LOOKUP_V, LOOKUP_INCRE = 3, 0.0025 / 64
UPSAMPLE_CASES = [(3, 32, 40, 128, 160), (2, 13, 21, 50, 77), (2, 1, 7, 5, 30), (2, 6, 1, 9, 1), (2, 9, 11, 9, 11), (1, 40, 50, 7, 9),
                  (5, 3, 5, 17, 3)]                          # (n, h, w, H, W)


def corr_case(C, r):
    """-> (f1, f2, coords, g): coordinates hashed over [-r-2, W2+r+1] x [-r-2, H2+r+1]; about a third of the samples inside the 2 x 2
    block of floor cells x in [2, 4), y in [4, 6) (texel (5, 3) lies in every footprint of those: a segment of >= 100 samples); the
    samples whose footprint would hold texel (0, 0) moved 2r + 2 texels to the right (a texel nobody samples); then, in both batch
    elements, planted samples: integral, exactly -1, exactly W2 - 1 / H2 - 1, NaN, +inf, 1e30, -3e9."""
    B, N, H1, W1, H2, W2 = (CORR_GEOM[k] for k in ("B", "N", "H1", "W1", "H2", "W2"))
    rd, seed = 2 * r + 1, 7000 + 10 * C + r
    f1, f2 = hashed((B, H1, W1, C), seed), hashed((B, H2, W2, C), seed + 1)
    g = hashed((B, N, rd * rd, H1, W1), seed + 2)
    x = hashed((B, N, H1, W1), seed + 3, -r - 2.0, W2 + r + 1.0)
    y = hashed((B, N, H1, W1), seed + 4, -r - 2.0, H2 + r + 1.0)
    crowd = hashed((B, N, H1, W1), seed + 5, 0.0, 1.0) < 0.36
    x = torch.where(crowd, hashed((B, N, H1, W1), seed + 6, 2.0, 3.999), x)
    y = torch.where(crowd, hashed((B, N, H1, W1), seed + 7, 4.0, 5.999), y)
    fx, fy = torch.floor(x), torch.floor(y)
    x = torch.where((fx >= -r - 1) & (fx <= r) & (fy >= -r - 1) & (fy <= r), x + (2 * r + 2.0), x)
    nan, inf = float("nan"), float("inf")
    plants = [((0, 0, 0), (3.0, 5.0)), ((1, 4, 6), (-1.0, 7.25)), ((2, 8, 12), (5.5, -1.0)), ((0, 8, 12), (W2 - 1.0, H2 - 1.0)),
              ((1, 0, 1), (nan, 2.5)), ((2, 3, 3), (2.5, inf)), ((0, 5, 7), (1e30, 2.5)), ((1, 7, 2), (2.5, -3e9)), ((2, 1, 9), (-3e9, nan)),
              ((0, 2, 2), (-inf, 4.5))]
    for (n, py, px), (vx, vy) in plants:
        x[:, n, py, px], y[:, n, py, px] = vx, vy
    return f1, f2, torch.stack([x, y], -1).contiguous(), g


def corr_census(coords, r, n2):
    """Edge counts of a correlation case from its coordinates and the reference's segment lengths n2 [B,H2,W2]."""
    x, y = coords[..., 0], coords[..., 1]
    H2, W2 = n2.shape[1:]
    fin = torch.isfinite(x) & torch.isfinite(y)
    return {"integral": int((fin & (x == torch.floor(x)) & (y == torch.floor(y))).sum()), "minus_one": int(((x == -1.0) | (y == -1.0)).sum()),
            "last_texel": int(((x == W2 - 1.0) & (y == H2 - 1.0)).sum()), "nan": int((torch.isnan(x) | torch.isnan(y)).sum()),
            "inf": int((torch.isinf(x) | torch.isinf(y)).sum()), "huge": int((fin & ((x.abs() > 2e9) | (y.abs() > 2e9))).sum()),
            "longest_segment": [int(v) for v in n2.reshape(n2.shape[0], -1).max(1).values],
            "empty_texels": [int(v) for v in (n2.reshape(n2.shape[0], -1) == 0).sum(1)]}


def assert_corr_census(cen, B=2):
    """What every correlation case must exercise (ISSUE: planted in both batch elements; census conditions)."""
    assert cen["integral"] >= B and cen["minus_one"] >= 2 * B and cen["last_texel"] >= B, cen
    assert cen["nan"] >= 2 * B and cen["inf"] >= 2 * B and cen["huge"] >= 2 * B, cen
    assert all(v >= 100 for v in cen["longest_segment"]) and all(v >= 1 for v in cen["empty_texels"]), cen


def lookup_case(D, L, r, P, shift):
    """-> (vol [V,D,P], origin [P], disp [P], gout [V, L (2r+1), P]): origin as TrainCorrBlock forms it (shift: the input disparity
    lifted to fl32(D//2 * incre)), disparities with c from the clamp up to 1.6 D as tests/test_train_step_gpu.py::_blocks, and four
    planted pixels: c clamped to exactly 0, c integral, c = D - 1 exactly (the last texel of level 0), c = D + r + 1 (every tap of level
    0 past the end).  A plant is found by stepping the disparity of a pixel ulp by ulp until the fp32 chain gives the value exactly."""
    V, seed = LOOKUP_V, 8000 + 16 * D + 2 * L + int(shift)
    incre = LOOKUP_INCRE
    vol = hashed((V, D, P), seed)
    gout = hashed((V, L * (2 * r + 1), P), seed + 1)
    d_in = hashed((P,), seed + 2, 0.0, 0.0025)
    lim = torch.tensor(D // 2 * incre, dtype=torch.float32)
    origin = torch.where(d_in < lim, lim, d_in) if shift else d_in.clone()
    disp = (origin + hashed((P,), seed + 3, -1.25 * D, 1.1 * D) * incre).contiguous()
    disp[0] = origin[0] - 2.0 * D * incre                                     # clamped to exactly 0
    disp[P - 1] = origin[P - 1]                                               # c = D // 2: integral (the last pixel: the partial block)
    for pix, target in ((P // 2, float(D - 1)), (P // 3 + 1, float(D + r + 1))):
        for cand in range(pix, P - 1):
            o = origin[cand:cand + 1]
            d = (o + (target - D // 2) * incre).clone()
            lo, hi = d.clone(), d.clone()
            hit = None
            for _ in range(64):
                for t in (lo, hi):
                    if float(tl_coord32(o, t, D, incre)) == target:
                        hit = t.clone()
                lo, hi = torch.nextafter(lo, lo - 1), torch.nextafter(hi, hi + 1)
                if hit is not None:
                    break
            if hit is not None:
                disp[cand] = hit[0]
                break
        else:                                                                 # (no pixel reaches the value: say so here, not in the census)
            raise AssertionError("lookup_case: no disparity gives c = %r at D = %d" % (target, D))
    return vol, origin, disp, gout


def lookup_census(origin, disp, D, L, r):
    c = tl_coord32(origin, disp, D, LOOKUP_INCRE)
    odd = [lv for lv in range(L) if (D >> lv) & 1]
    # the fold's guard fires for element d of level 0 and level lv when d >> lv == D >> lv
    guard = sum(int(((torch.arange(D) >> lv) >= (D >> lv)).sum()) for lv in range(1, L))
    return {"clamped": int((c == 0).sum()), "integral": int((c == torch.floor(c)).sum()), "last_texel": int((c == float(D - 1)).sum()),
            "past_end": int((c == float(D + r + 1)).sum()), "beyond": int((c > D + r).sum()), "odd_levels": odd, "guarded_elements": guard,
            "partial_block": origin.numel() % 64}


def assert_lookup_census(cen, D, L, P):
    assert cen["clamped"] >= 1 and cen["integral"] >= 2 and cen["last_texel"] >= 1 and cen["past_end"] >= 1 and cen["beyond"] >= 1, cen
    needs_guard = any(((D >> (lv - 1)) & 1) for lv in range(1, L))            # an odd length at a level that is pooled further
    assert (cen["guarded_elements"] > 0) == needs_guard, cen
    assert cen["partial_block"] == P % 64, cen


def upsample_case(n, h, w, H, W):
    """-> (x [n,h,w], g [n,H,W])"""
    seed = 9000 + 31 * h + w
    return hashed((n, h, w), seed), hashed((n, H, W), seed + 1)


def upsample_census(h, w, H, W):
    """Edge counts of an upsample case, from the brute-force range tables alone."""
    ry, rx = upsample_ranges_brute(h, H), upsample_ranges_brute(w, W)
    ly, lx = ry[:, 1] - ry[:, 0], rx[:, 1] - rx[:, 0]
    return {"empty_rows": int((ly == 0).sum()), "empty_cols": int((lx == 0).sum()), "longest_range": (int(ly.max()), int(lx.max())),
            "one_texel_axis": (h == 1, w == 1), "one_output_axis": (H == 1, W == 1), "identity": (h, w) == (H, W)}


# What every upsample case exercises, in the order of UPSAMPLE_CASES: both modules assert the whole dict of every case, so that a case
# cannot stop reaching its edge unnoticed.  An axis with one texel has one range over every output (5 rows in the third case); an axis
# with one output reads texel 0 alone; the identity's ranges have two outputs (X = j through i0 and X = j - 1 through i1 with weight 0);
# the downsampling case leaves 27 rows and 33 columns in no footprint (7 and 9 outputs touch at most 14 and 18 texels, fewer where
# two outputs share one).
def _census(empty, longest, one_texel=(False, False), one_output=(False, False), identity=False):
    return {"empty_rows": empty[0], "empty_cols": empty[1], "longest_range": longest, "one_texel_axis": one_texel,
            "one_output_axis": one_output, "identity": identity}


UPSAMPLE_CENSUS = dict(zip(UPSAMPLE_CASES, [
    _census((0, 0), (9, 9)), _census((0, 0), (9, 8)), _census((0, 0), (5, 10), one_texel=(True, False)),
    _census((0, 0), (4, 1), one_texel=(False, True), one_output=(False, True)), _census((0, 0), (2, 2), identity=True),
    _census((27, 33), (1, 1)), _census((0, 0), (16, 1))]))
