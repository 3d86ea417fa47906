"""The restated fp32 coordinates of the cost volume (``parity_check.fma32`` / ``cost_coords32``), the geometries of
tests/cost_geometry_cases.py and the per-element check of tests/test_cost_geometry_gpu.py, on the CPU.

  * ``fma32`` against fractions.Fraction: 12 000 hashed triples over 40 binades, the constructed float32 ties on which a float64 sum rounds
    twice, and exact cancellations.
  * ``cost_coords32`` against the float64 projection of ``cost_volume_ref64`` within the fp32 conditioning of each coordinate (bound
    stated in the test's docstring), origins bit-equal to ``O.hypothesis_origin``; ``cost_samples_ref64`` against ``cost_volume_ref64``
    on the four benign walk geometries within slope x coordinate difference.
  * The conditions the new geometries must meet BY CONSTRUCTION (checked on the reference alone - no kernel output chose a constant), and
    the census of the old ones next to them (printed; DESIGN.md section 4 holds the table).
  * Eight planted corruptions in an fp32 torch emulation of the volume built from the restated coordinates: each fails the new check, the
    report names the pixel, tile, row or seam, and OLD_CRITERION_PASSES records what ``4e-6 * max(|vol|, 1)`` over the matrix - the
    criterion of test_cost_lines_matches_walk - makes of it.
"""
import fractions

import numpy as np
import pytest
import torch

import cost_geometry_cases as G
import parity_check as pc
import wide_parity_cases as wide
from test_oracle_golden import hashed

F = fractions.Fraction


# ------------------------------------------------------------------------------------------------ fma32
def round_fraction_f32(q):
    """The float32 nearest the rational q, ties to even (subnormals included; no overflow in these tests)."""
    if q == 0:
        return np.float32(0.0)
    sign, q = (-1, -q) if q < 0 else (1, q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if F(2) ** e > q:
        e -= 1                                               # 2^e <= q < 2^(e + 1)
    ulp = F(2) ** (max(e, -126) - 23)
    n = q / ulp
    fl = n.numerator // n.denominator
    rem = n - fl
    if rem > F(1, 2) or (rem == F(1, 2) and fl % 2 == 1):
        fl += 1
    return np.float32(sign * float(fl * ulp))                # (fl * ulp has <= 24 significant bits: exact in a double, then in a float32)


def _same_f32(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.int32), np.asarray(b, dtype=np.float32).view(np.int32))


def test_fma32_is_exact_on_hashed_triples():
    n = 12000
    ex = lambda seed: np.exp2(np.round(hashed((n,), seed, -20, 20).numpy())).astype(np.float32)
    a = hashed((n,), 5101).numpy() * ex(5102)
    b = hashed((n,), 5103).numpy() * ex(5104)
    c = hashed((n,), 5105).numpy() * ex(5106)
    third = np.arange(n) % 3
    with np.errstate(all="ignore"):
        c = np.where(third == 1, -(a * b).astype(np.float32) * np.float32(1 + 2.0 ** -20), c).astype(np.float32)      # heavy cancellation
        c = np.where(third == 2, (a * b).astype(np.float32) * np.float32(2.0 ** 24), c).astype(np.float32)            # the product barely counts
    got = pc.fma32(a, b, c)
    want = np.array([round_fraction_f32(F(float(x)) * F(float(y)) + F(float(z))) for x, y, z in zip(a, b, c)], dtype=np.float32)
    bad = got.view(np.int32) != want.view(np.int32)
    assert not bad.any(), (int(bad.sum()), a[bad][:3], b[bad][:3], c[bad][:3], got[bad][:3], want[bad][:3])
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    print(f"  fma32: {n} triples exact; the float64 sum rounded to float32 differs on {int((naive.view(np.int32) != want.view(np.int32)).sum())}")


def test_fma32_on_constructed_ties_and_cancellations():
    """p = a b = 2^-24 (1 - 2^-46): in float64, c + p rounds to the midpoint of c and its float32 neighbour, and a second rounding to
    even then goes UP for odd c although the true sum lies below the midpoint.  Both signs, 64 mantissas, several binades."""
    wrong_naive = 0
    for scale in (0, 7, -9, -100):                           # (-100: c near 2^-100, still normal)
        for j in range(64):
            for sign in (1.0, -1.0):
                a = np.float32((1 + 2.0 ** -23) * 2.0 ** (scale - 12))
                b = np.float32((1 - 2.0 ** -23) * 2.0 ** -12)
                c = np.float32(sign * (1 + j * 2.0 ** -23) * 2.0 ** scale)
                want = round_fraction_f32(F(float(a)) * F(float(b)) + F(float(c)))
                assert _same_f32(pc.fma32(a, b, c), want), (scale, j, sign)
                wrong_naive += not _same_f32(np.float32(np.float64(a) * np.float64(b) + np.float64(c)), want)
                # exact cancellation: fma(a, b, -fl(a b)) is the product's own rounding error, representable
                x, y = np.float32(1 + (2 * j + 1) * 2.0 ** -23), np.float32((1 + 3 * 2.0 ** -22) * 2.0 ** scale)
                p = np.float32(x * y)
                r = pc.fma32(x, y, -p)
                assert F(float(r)) == F(float(x)) * F(float(y)) - F(float(p)), (scale, j)
    assert wrong_naive >= 64                                 # the construction does hit the double rounding fma32 is there to avoid
    # subnormal results and signed zeros
    assert _same_f32(pc.fma32(np.float32(2.0 ** -100), np.float32(2.0 ** -49), np.float32(0)), np.float32(2.0 ** -149))
    assert _same_f32(pc.fma32(np.float32(2.0 ** -100), np.float32(2.0 ** -50), np.float32(0)), np.float32(0.0))          # a tie to even: 0
    assert _same_f32(pc.fma32(np.float32(3 * 2.0 ** -100), np.float32(2.0 ** -50), np.float32(0)), np.float32(2.0 ** -148))      # 1.5 steps: a tie, to 2
    assert _same_f32(pc.fma32(np.float32(3 * 2.0 ** -100), np.float32(2.0 ** -50), np.float32(-2.0 ** -149)), np.float32(0.0))   # 0.5 steps: a tie, to 0
    assert _same_f32(pc.fma32(np.float32(2.0), np.float32(3.0), np.float32(-6.0)), np.float32(0.0))


# ------------------------------------------------------------------------------------------------ the coordinates
SMALL_CASES = [c for c in G.CASES if (c[3], c[4]) != G.BIG]


def test_coords32_against_the_float64_projection_and_the_oracle_origins():
    """How far a correct fp32 evaluation of u = X / Z may lie from the float64 one: X32 = fma(m3, hyp32, fl(fma(m1, y, fl(m0 x)) + m2))
    takes four roundings, each of a partial sum that is at most T = |m0 x| + |m1 y| + |m2| + |m3 hyp|, and hyp32 itself is one rounding
    from the float64 hyp (|m3 hyp| u more): eX = 5 u T to first order, taken twice that; the same for Z; then
    |u32 - u64| <= (eX + |u64| eZ) / (|Z64| - eZ) + 2 u |u64| (the division's own rounding), wherever |Z64| > 8 eZ and the clamp is not
    reached.  Origins: bit-equal to O.hypothesis_origin."""
    from oracle import cer_oracle as O
    u24 = 2.0 ** -24
    worst = 0.0
    for geom, D, stage0, h, w in SMALL_CASES:
        _, Pij, d0 = G.lines_geometry(geom, D, stage0, h, w)
        incre = G.incre_of(stage0)
        co = G.coords(geom, D, stage0, h, w)
        assert np.array_equal(co["origin"].view(np.int32), O.hypothesis_origin(d0, D, incre, stage0).numpy().view(np.int32)), (geom, D, h, w)
        # the float64 projection, as cost_volume_ref64 forms it
        steps = ((torch.arange(D) - D // 2) * incre).to(torch.float32).double()
        hyp = steps[None, :] + torch.from_numpy(co["origin"]).double()[:, None]
        x, y = (torch.arange(h * w) % w).double()[:, None], (torch.arange(h * w) // w).double()[:, None]
        for v in range(G.V):
            m = Pij[v].double()
            val = lambda r: m[r, 0] * x + m[r, 1] * y + m[r, 2] + m[r, 3] * hyp
            T = lambda r: (m[r, 0] * x).abs() + (m[r, 1] * y).abs() + m[r, 2].abs() + (m[r, 3] * hyp).abs()
            X, Y, Z = val(0), val(1), val(2)
            eX, eY, eZ = (2 * 5 * u24 * T(r) for r in range(3))
            for c32, N, eN in ((co["u"][v], X, eX), (co["t"][v], Y, eY)):
                q = N / Z
                use = (Z.abs() > 8 * eZ) & (q.abs() < 9.9e3)                      # (conditioned, and not at the clamp)
                bound = (eN + q.abs() * eZ) / (Z.abs() - eZ).clamp_min(1e-300) + 2 * u24 * q.abs()
                ratio = ((torch.from_numpy(c32).double() - q).abs() / bound.clamp_min(1e-300))[use]
                assert use.any() or geom in ("zero_over_zero",)
                if ratio.numel():
                    worst = max(worst, float(ratio.max()))
                    assert float(ratio.max()) <= 1.0, (geom, D, h, w, v, float(ratio.max()))
    print(f"  cost_coords32 vs float64: worst |difference| / conditioning bound over {len(SMALL_CASES)} cases: {worst:.3f}")


def test_samples_ref64_agrees_with_cost_volume_ref64_on_the_benign_walk_geometries():
    """Same definition, coordinates formed in fp32 instead of float64: the values differ by at most slope x coordinate difference, the
    slope of a bilinear interpolant being at most 2 max|texel dot| <= 2 sum_c |f1_c| max_texel |f2_c| per texel of displacement.  The
    position a sample is taken at is cell + fraction: at negative coordinates the fp32 fraction u - floor(u) is itself rounded (2^-25)."""
    worst = 0.0
    for geom in wide.WALK_GEOMS:
        for stage, D in ((0, 64), (1, 44)):
            h, w, V = 19, 45, 3
            c = wide.walk_case(geom, stage, h, w, V)
            ref, norm, _ = pc.cost_volume_ref64(c["fmaps"], c["Pij"], D, c["incre"], c["disp_in"], c["shift"])
            co = pc.cost_coords32(c["Pij"], D, c["incre"], c["disp_in"].reshape(-1), c["shift"], h, w)
            f1, f2 = G.rows_of(c["fmaps"])
            S = pc.cost_samples_ref64(f1, f2, co)
            # float64 coordinates
            steps = ((torch.arange(D) - D // 2) * c["incre"]).to(torch.float32).double()
            hyp = steps[None, :] + torch.from_numpy(co["origin"]).double()[:, None]
            x, y = (torch.arange(h * w) % w).double()[:, None], (torch.arange(h * w) // w).double()[:, None]
            slope = 2 * (f1.double().abs() * f2.double().abs().amax((1, 2))[:, None, :]).sum(-1)              # [V, P]
            for v in range(V):
                m = c["Pij"][v].double()
                val = lambda r: m[r, 0] * x + m[r, 1] * y + m[r, 2] + m[r, 3] * hyp
                pos = lambda cell, frac: torch.from_numpy(co[cell][v]).double() + torch.from_numpy(co[frac][v]).double()
                du = (pos("iu", "du") - val(0) / val(2)).abs() + (pos("iw", "dw") - val(1) / val(2)).abs()
                bound = slope[v][:, None] * du + 1e-12
                ratio = (S["val"][v] - ref[v]).abs() / bound
                worst = max(worst, float(ratio.max()))
                assert float(ratio.max()) <= 1.0, (geom, stage, v, float(ratio.max()))
                assert float((S["norm"][v] - norm[v]).abs().max()) <= float((slope[v][:, None] * du).max()) + 1e-12
    print(f"  cost_samples_ref64 vs cost_volume_ref64: worst |difference| / (slope x coordinate difference) {worst:.3f}")


# ------------------------------------------------------------------------------------------------ conditions, not measurements
def test_geometry_conditions_and_census():
    widest = 0.0
    for geom, D, stage0, h, w in SMALL_CASES:
        cs = G.census(geom, D, stage0, h, w)
        widest = max(widest, max(c["band"] for c in cs))
        line = " | ".join(f"{c['in_map']:.2f} z+-{c['z_sign']:.2f} nan {c['not_ok']} graze {c['graze']} band {c['band']:.0f}" for c in cs)
        print(f"  {G.case_id(geom, D, stage0, h, w):32s} {line}")
        tag = (geom, D, h, w)
        if geom in G.NEW_GEOMS:
            assert sum(c["in_map"] >= 0.25 for c in cs) >= 2, tag
        if geom == "wild_in_map":
            assert any(c["z_sign"] >= 0.10 and c["in_map_pos"] >= 0.05 and c["in_map_neg"] >= 0.05 for c in cs), tag
            assert cs[2]["z_sign"] == 0.0 and cs[2]["in_map_pos"] == 0.0 and cs[2]["in_map"] >= 0.25, tag      # entirely behind the camera, in the map
        if geom == "zero_over_zero":
            assert sum(c["not_ok"] for c in cs) >= 8, tag
        if geom == "border_graze":
            assert sum(c["graze"] for c in cs) >= 200, tag
            co = G.coords(geom, D, stage0, h, w)
            assert (co["iu"][2] < -2).any() and (co["iw"][2] > h).any(), tag                                  # beyond the texel clamp, both ends
            assert ((co["iu"][0] == -1) & co["ok"][0]).mean() > 0.25 and ((co["iu"][1] == w - 1) & co["ok"][1]).mean() > 0.25, tag
        if geom == "forward":
            assert all(c["epipole_inside"] for c in cs), tag
        if geom == "rotation":
            assert all(c["one_cell"] for c in cs), tag
    assert widest > 29.0, widest
    # the table of the issue reproduces (share of the samples in the map, per view)
    near = lambda c, want: all(abs(a["in_map"] - b) <= 0.015 for a, b in zip(c, want))
    assert near(G.census("wild", 44, False, 19, 45), (0.08, 0.00, 0.00)) and near(G.census("wild", 20, False, 33, 65), (0.08, 0.00, 0.00))
    assert near(G.census("wild", 64, True, 19, 45), (0.20, 0.10, 0.00)) and near(G.census("vertical", 44, False, 19, 45), (0.56, 0.19, 0.08))
    assert all(0.015 <= c["in_map"] <= 0.045 for hw in ((19, 45), (33, 65)) for D, s0 in G.DS for c in G.census("zoom", D, s0, *hw))


# ------------------------------------------------------------------------------------------------ planted corruptions
# True: 4e-6 * max(|vol|, 1) over the whole matrix (test_cost_lines_matches_walk) passes the corruption - it is invisible to it.
OLD_CRITERION_PASSES = {
    "texel_off": False,
    "lo_plane_dropped_in_one_tile": False,               # (4.5e-6 against 4e-6 * 1: by a hair, as one maximum that names no tile)
    "nan_sampled_at_the_clamp": False,
    "y0_ignored_in_the_last_row": False,
    "texel_clamp_off_by_one": False,
    "view_skipped_in_one_segment": False,
    "level2_from_unscaled_level0": False,
    "view2_reads_slot1": False,
}


def emulate(f1, f2, co, scale, num_levels=3, compact=True, views=None, edit=None):
    """The volume rows in torch float32 from restated coordinates ``co``: four texel dots, fp32 weights, view sum in view order, scale,
    pooled levels.  ``edit(v, iu, iw, du, dw, ok)`` may return changed copies of a view's sample arrays (a planted addressing error);
    ``views``: which source map each view reads.  -> (rows [P, rs], the per-view values [P, D])."""
    from cer_mvs_amd import ops
    V, P, D = co["ok"].shape
    h2, w2, C = f2.shape[1:]
    views = list(range(V)) if views is None else views
    f1 = f1.float()
    tt = torch.from_numpy
    total = torch.zeros(P, D)
    parts = []
    for v in range(V):
        f2z = torch.cat([f2[views[v]].float().reshape(-1, C), torch.zeros(1, C)], 0)
        iu, iw, du, dw, ok = tt(co["iu"][v]).long(), tt(co["iw"][v]).long(), tt(co["du"][v]), tt(co["dw"][v]), tt(co["ok"][v])
        if edit is not None:
            iu, iw, du, dw, ok = edit(v, iu, iw, du, dw, ok)
        val = torch.zeros(P, D)
        for dy, dx in pc.CORNERS:
            wt = (du if dx else 1.0 - du) * (dw if dy else 1.0 - dw)
            xi, yi = iu + dx, iw + dy
            inside = ok & (xi >= 0) & (xi < w2) & (yi >= 0) & (yi < h2)
            idx = torch.where(inside, yi * w2 + xi, torch.full_like(xi, h2 * w2))
            val = val + torch.einsum("pdc,pc->pd", f2z[idx], f1) * wt
        parts.append(val)
        total = total + val
    offs, lens, rs = ops.row_layout(D, num_levels, compact)
    rows = torch.zeros(P, rs)
    cur = total * np.float32(scale)
    rows[:, :D] = cur
    for l in range(1, 1 if compact else num_levels):
        n = cur.shape[1] // 2
        cur = (cur[:, 0:2 * n:2] + cur[:, 1:2 * n:2]) * 0.5
        rows[:, offs[l]:offs[l] + lens[l]] = cur
    return rows, parts


def old_passes(bad, clean, D):
    return float((bad[:, :D] - clean[:, :D]).abs().max()) <= 4e-6 * max(float(clean[:, :D].abs().max()), 1.0)


@pytest.mark.parametrize("geom", G.NEW_GEOMS + ["zoom", "wild", "forward"])
def test_the_clean_emulation_passes(geom):
    """The fp32 emulation (torch's 64-term dot) against the reference, at the three-term bound and full rows."""
    for D, stage0 in G.DS:
        h, w = 19, 45
        fm, _, _ = G.lines_geometry(geom, D, stage0, h, w)
        f1, f2 = G.rows_of(fm)
        R = pc.cost_rows_ref64(G.samples(geom, D, stage0, h, w), D, 3, 1.0 / G.V, False)
        rows, _ = emulate(f1, f2, G.coords(geom, D, stage0, h, w), 1.0 / G.V, compact=False)
        rep = pc.check_cost_rows(rows, R, G.V, "three-term", f"clean {geom} D={D}", h, w)
        assert rep.ok, rep.message()


def _three_term(geom, D, stage0, h, w, compact=True):
    fm, _, _ = G.lines_geometry(geom, D, stage0, h, w)
    f1, f2 = G.rows_of(fm)
    co = G.coords(geom, D, stage0, h, w)
    R = pc.cost_rows_ref64(G.samples(geom, D, stage0, h, w), D, 3, 1.0 / G.V, compact)
    clean, _ = emulate(f1, f2, co, 1.0 / G.V, compact=compact)
    assert pc.check_cost_rows(clean, R, G.V, "three-term", "clean", h, w).ok
    return f1, f2, co, R, clean


def test_one_sample_one_texel_off():
    """1. One in-map sample of ``zoom`` reads the cell to its right."""
    D, h, w = 64, 19, 45
    f1, f2, co, R, clean = _three_term("zoom", D, True, h, w)
    inm = co["ok"][0] & (co["iu"][0] >= 1) & (co["iu"][0] < w - 3) & (co["iw"][0] >= 1) & (co["iw"][0] < h - 2)
    pix, k = [int(t) for t in np.argwhere(inm)[len(np.argwhere(inm)) // 2]]

    def edit(v, iu, iw, du, dw, ok):
        if v == 0:
            iu = iu.clone()
            iu[pix, k] += 1
        return iu, iw, du, dw, ok
    bad, _ = emulate(f1, f2, co, 1.0 / G.V, edit=edit)
    rep = pc.check_cost_rows(bad, R, G.V, "three-term", "texel off", h, w)
    assert rep.n_fail == 1 and rep.pixels.tolist() == [pix] and rep.worst == (pix // w, pix % w, k) and f"row {pix // w}, column {pix % w}" in rep.message()
    assert old_passes(bad, clean, D) == OLD_CRITERION_PASSES["texel_off"]


def test_lo_plane_dropped_in_one_tile_of_small_values():
    """2. One 32-pixel tile reads the source rows as f16 (x * 64 rounded to 11 bits: 2^-12 relative per product) where the reference rows
    are 1 / 8 of their size elsewhere.  The condition on ``cost_bound``: this must be visible."""
    geom, D, h, w = "zoom_in_map", 64, 19, 45
    fm, _, _ = G.lines_geometry(geom, D, True, h, w)
    f1, f2 = G.rows_of(fm)
    co = G.coords(geom, D, True, h, w)
    tile = torch.zeros(h, w, dtype=torch.bool)
    tile[11, 0:32] = True
    tile = tile.reshape(-1)
    f1 = torch.where(tile[:, None], f1 * 0.125, f1)
    R = pc.cost_rows_ref64(pc.cost_samples_ref64(f1, f2, co), D, 3, 1.0 / G.V, True)
    clean, _ = emulate(f1, f2, co, 1.0 / G.V)
    assert pc.check_cost_rows(clean, R, G.V, "three-term", "clean", h, w).ok
    dropped, _ = emulate(f1, pc.cost_f2_two_term(f2), co, 1.0 / G.V)
    bad = torch.where(tile[:, None], dropped, clean)
    rep = pc.check_cost_rows(bad, R, G.V, "three-term", "lo plane dropped", h, w)
    assert not rep.ok and rep.only_tile() == (11, 0) and "confined to tile (11, 0)" in rep.message() and rep.n_fail > 32
    print(f"  lo plane dropped in one tile: {rep.n_fail} of {32 * D} elements of the tile fail, worst |err| / bound {rep.max_ratio:.2f}")
    assert old_passes(bad, clean, D) == OLD_CRITERION_PASSES["lo_plane_dropped_in_one_tile"], float((bad - clean).abs().max())


def test_nan_sample_taken_at_the_clamp():
    """3. A 0 / 0 sample is not zeroed: its coordinates are taken for the clamped corner of the map (cell (0, 0), weight 1)."""
    geom, D, h, w = "zero_over_zero", 44, 19, 45
    f1, f2, co, R, clean = _three_term(geom, D, False, h, w)
    nans = np.argwhere(~co["ok"][0])

    def edit(v, iu, iw, du, dw, ok):
        if v == 0:
            iu, iw = torch.where(ok, iu, torch.zeros_like(iu)), torch.where(ok, iw, torch.zeros_like(iw))
            ok = torch.ones_like(ok)
        return iu, iw, du, dw, ok
    bad, _ = emulate(f1, f2, co, 1.0 / G.V, edit=edit)
    rep = pc.check_cost_rows(bad, R, G.V, "three-term", "NaN sampled", h, w)
    assert not rep.ok and set(rep.pixels.tolist()) <= set(nans[:, 0].tolist()) and set(rep.channels) == {D // 2} and rep.n_fail >= len(nans) - 2
    assert old_passes(bad, clean, D) == OLD_CRITERION_PASSES["nan_sampled_at_the_clamp"]


def test_y0_ignored_in_the_last_row_of_a_slab():
    """4. Rows 5 .. h - 1 as a slab: its last row is projected with py = y instead of y + y0."""
    geom, D, h, w, y0 = "wild_in_map", 20, 19, 45, 5
    fm, Pij, d0 = G.lines_geometry(geom, D, False, h, w)
    f1, f2 = G.rows_of(fm)
    co = G.coords(geom, D, False, h, w, y0, None)
    R = pc.cost_rows_ref64(G.samples(geom, D, False, h, w, False, y0, None), D, 3, 1.0 / G.V, True)
    hs = h - y0
    clean, _ = emulate(f1[y0 * w:], f2, co, 1.0 / G.V)
    assert pc.check_cost_rows(clean, R, G.V, "three-term", "clean slab", hs, w).ok
    wrong = pc.cost_coords32(Pij, D, G.incre_of(False), d0[y0 * w:], False, hs, w, y0=0)
    mixed = {k: (np.concatenate([co[k][:, :(hs - 1) * w], wrong[k][:, (hs - 1) * w:]], 1) if k not in ("hyp", "origin") else co[k]) for k in co}
    bad, _ = emulate(f1[y0 * w:], f2, mixed, 1.0 / G.V)
    rep = pc.check_cost_rows(bad, R, G.V, "three-term", "y0 ignored", hs, w)
    assert not rep.ok and rep.only_row() == hs - 1 and "(the last row)" in rep.message()
    assert old_passes(bad, clean, D) == OLD_CRITERION_PASSES["y0_ignored_in_the_last_row"]


def test_texel_clamp_off_by_one():
    """5. Cells at u in (-1, 0) are clamped to column 0 instead of -1: the sample reads columns 0 | 1 where it should read border | 0."""
    geom, D, h, w = "border_graze", 44, 19, 45
    f1, f2, co, R, clean = _three_term(geom, D, False, h, w)

    def edit(v, iu, iw, du, dw, ok):
        return iu.clamp_min(0), iw, du, dw, ok
    bad, _ = emulate(f1, f2, co, 1.0 / G.V, edit=edit)
    rep = pc.check_cost_rows(bad, R, G.V, "three-term", "clamp off by one", h, w)
    touched = set(np.argwhere(((co["iu"] == -1) & co["ok"]).any((0, 2))).reshape(-1).tolist())
    assert not rep.ok and set(rep.pixels.tolist()) <= touched and rep.n_fail > 200
    assert old_passes(bad, clean, D) == OLD_CRITERION_PASSES["texel_clamp_off_by_one"]


def test_one_view_skipped_in_one_segment():
    """6. The second 32-pixel segment of one image row misses view 1 in its sum."""
    geom, D, h, w = "zoom_in_map", 20, 33, 65
    f1, f2, co, R, clean = _three_term(geom, D, False, h, w)
    _, parts = emulate(f1, f2, co, 1.0 / G.V)
    seg = torch.zeros(h, w, dtype=torch.bool)
    seg[17, 32:64] = True
    seg = seg.reshape(-1)
    bad = clean.clone()
    bad[seg, :D] = ((parts[0] + parts[2]) * np.float32(1.0 / G.V))[seg]
    rep = pc.check_cost_rows(bad, R, G.V, "three-term", "view skipped", h, w)
    assert not rep.ok and rep.only_tile() == (17, 1) and rep.on_seam >= 1 and set(rep.cols) <= set(range(32, 64))
    assert old_passes(bad, clean, D) == OLD_CRITERION_PASSES["view_skipped_in_one_segment"]


def test_pooled_level_2_from_the_unscaled_level_0():
    """7. Full rows: level 2 is pooled from the view SUM, levels 0 and 1 from the view mean."""
    geom, D, h, w = "wild_in_map", 44, 19, 45
    f1, f2, co, R, clean = _three_term(geom, D, False, h, w, compact=False)
    unscaled, _ = emulate(f1, f2, co, 1.0, compact=False)
    lvl2 = (R["level"] == 2).nonzero().reshape(-1)
    bad = clean.clone()
    bad[:, lvl2] = unscaled[:, lvl2]
    rep = pc.check_cost_rows(bad, R, G.V, "three-term", "level 2 unscaled", h, w)
    assert not rep.ok and set(rep.channels) <= set(lvl2.tolist()) and len(rep.channels) == len(lvl2)
    assert old_passes(bad, clean, D + D // 2 + D // 4) == OLD_CRITERION_PASSES["level2_from_unscaled_level0"]


def test_view_2_reads_the_slot_of_view_1():
    """8. The gathered buffer: view 2 samples source map 1."""
    geom, D, h, w = "border_graze", 20, 7, 13
    f1, f2, co, R, clean = _three_term(geom, D, False, h, w)
    bad, _ = emulate(f1, f2, co, 1.0 / G.V, views=[0, 1, 1])
    rep = pc.check_cost_rows(bad, R, G.V, "three-term", "view 2 reads slot 1", h, w)
    inm2 = set(np.argwhere((co["ok"][2] & (co["iu"][2] >= -1) & (co["iu"][2] < w) & (co["iw"][2] >= -1) & (co["iw"][2] < h)).any(1)).reshape(-1).tolist())
    assert not rep.ok and set(rep.pixels.tolist()) <= inm2 and len(set(rep.pixels.tolist())) > len(inm2) // 2
    assert old_passes(bad, clean, D) == OLD_CRITERION_PASSES["view2_reads_slot1"]
