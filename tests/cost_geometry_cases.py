"""The inputs of tests/test_cost_geometry_gpu.py, shared with tests/test_cost_geometry_cpu.py (which checks the restatement, the conditions
the geometries must meet and what the per-element check makes of planted corruptions) and with tests/test_hip_parity.py, whose
``_lines_case`` is a thin wrapper around ``lines_geometry``.  CPU tensors only, deterministic, the same on every machine; every float64
reference is computed once per case (functools.lru_cache; the large ones keep the last few cases only) and handed out unchanged - nobody
writes into what these functions return.

Geometries.  The eight of test_cost_lines_matches_walk stay as they are (OLD_GEOMS: the very code that stood in ``_lines_case``).  Two of
them exist to drive the tile kernel's per-sample direct path and its hand-over list, and sample almost nothing but the zero border
(``census``: zoom 0.03, wild 0.00 - 0.20 of their samples in the map).  NEW_GEOMS put signal on those paths; they are built in STEP units -
s = (hyp - hc) / incre, hc the centre of the hypothesis range - so that one description serves every (D, stage):
  zoom_in_map     the same 6 x magnification (Pij[0, 0] = Pij[1, 1] = 6), recentred on the image corner and under a perspective row
                  Z = 1 + 5 x / w + 5 y / h that brings the far end back: six texels per pixel at the corner, every sample in the map;
  wild_in_map     Z = zs (s - kappa(pixel)) crosses 0 inside the hypothesis range for the inner 60 % of the image (view 0: kappa along x,
                  view 1: along y) and X = cx Z + ex, Y = cy Z + ey, so that u = cx + ex / Z stays finite and in the map on BOTH sides of
                  the crossing; view 2 lies entirely behind the camera (Z < 0) and still samples the map (X, Y negated too);
  zero_over_zero  Z = hyp - H with H the origin of the un-jittered pixels: Z is EXACTLY 0 at k = D // 2; X = cx Z + g (x - y) (view 0) and
                  Y = cy Z + g (x - 2 y) (view 1) with cx, cy, g powers of two vanish exactly on a line of pixels: 0 / 0, a genuine NaN
                  (elsewhere on that hypothesis: +-inf, clamped to +-1e4);
  border_graze    Z = 1; view 0 sweeps u over (-1.5, 0.4) and spreads t over (-0.8, h - 0.3), view 1 does the same at the right and
                  bottom borders, view 2 runs from four texels outside to inside on both axes (the [-2, w2] texel clamp).
Their hypothesis origins carry a +-1.5-step hashed jitter; at stage 0 half of them lie below lim and take the shift rule."""
import functools
import math

import numpy as np
import torch

import parity_check as pc
from test_oracle_golden import hashed

V, C = 3, 64
OLD_GEOMS = ["horizontal", "diagonal", "vertical", "wild", "rotation", "forward", "converging", "zoom"]
NEW_GEOMS = ["zoom_in_map", "wild_in_map", "zero_over_zero", "border_graze"]
GEOMS = OLD_GEOMS + NEW_GEOMS
# The smallest sizes at which the 32-pixel sheared tiles can go wrong: 7 x 13 shorter than a tile on both axes; 19 x 45 a partial second
# segment along x; 33 x 65 one pixel into the second / third segment on both axes (views whose tile axis is y); 70 x 150 (BIG_GEOMS only)
# interior tiles and several segments.
SIZES = [(7, 13), (19, 45), (33, 65)]
BIG = (70, 150)
BIG_GEOMS = ["diagonal", "converging"]
DS = [(64, True), (44, False), (20, False)]                 # (D, stage0)
D_ODD = 37                                                  # not a multiple of 4: row_layout pads the row to 40, both builders accept it
CASES = [(g, D, s0, h, w) for g in GEOMS for D, s0 in DS for h, w in SIZES + ([BIG] if g in BIG_GEOMS else [])]


def incre_of(stage0):
    return 0.0025 / (64 if stage0 else 320)


def case_id(geom, D, stage0, h, w):
    return f"{geom}-D{D}-{h}x{w}"


# ------------------------------------------------------------------------------------------------ the geometries
def _old_pij(geom, stage0, h1, w1):
    """The eight geometries of test_cost_lines_matches_walk, exactly as ``_lines_case`` built them."""
    Pij = torch.eye(4).repeat(V, 1, 1)
    for v in range(V):
        if geom == "horizontal":
            Pij[v, 0, 3] = (900.0 if stage0 else 9000.0) * (v + 1) * (1 if v != 1 else -1)
        elif geom == "vertical":
            Pij[v, 1, 3] = -(700.0 if stage0 else 7000.0) * (v + 1)
        elif geom == "diagonal":
            Pij[v, 0, 3], Pij[v, 1, 3] = 600.0 * (v + 1), (-500.0, 450.0, -80.0)[v] * (v + 1)
            Pij[v, 0, 1] = 0.05 * v
        elif geom == "rotation":          # no baseline: every hypothesis of a pixel lands on one point (+ a small homography)
            Pij[v, 0, 1], Pij[v, 1, 0], Pij[v, 0, 2], Pij[v, 1, 2] = 0.02 * v, -0.02 * v, 1.3 * v, -0.7
        elif geom == "forward":           # epipole inside the image: lines of every direction within one view
            Pij[v, 0, 3], Pij[v, 1, 3], Pij[v, 2, 3] = 0.5 * w1 * 400.0, 0.5 * h1 * 400.0, 400.0 * (v + 1)
        elif geom == "converging":        # rotation + baseline (the bench scene's kind of pair): the epipole is finite, far away
            th = 0.12 * (v + 1) * (1 if v % 2 else -1)
            f = 1.8 * w1
            K = torch.tensor([[f, 0, w1 / 2], [0, f, h1 / 2], [0, 0, 1.0]])
            R = torch.tensor([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]], dtype=torch.float32)
            Rx = torch.tensor([[1, 0, 0], [0, np.cos(0.04 * v), -np.sin(0.04 * v)], [0, np.sin(0.04 * v), np.cos(0.04 * v)]], dtype=torch.float32)
            R = Rx @ R
            c = torch.tensor([0.0, 0.0, 600.0])
            Pij[v, :3, :3] = K @ R @ torch.linalg.inv(K)
            Pij[v, :3, 3] = K @ (c - R @ c)
        elif geom == "zoom":              # source view magnified 6x: neighbouring lines are 6 texels apart (eight-line form: todo list)
            Pij[v, 0, 0] = Pij[v, 1, 1] = 6.0
            Pij[v, 0, 2], Pij[v, 1, 2] = -2.5 * w1, -2.5 * h1
            Pij[v, 0, 3] = (2500.0 if stage0 else 25000.0) * (v + 1)
            Pij[v, 1, 3] = 300.0 * v
        else:   # wild: Z = 1 + m[11] * hyp crosses zero inside the range; one view entirely behind the camera
            Pij[v, 0, 3], Pij[v, 2, 3] = 4000.0, (-700.0, -1500.0, 0.0)[v]
            if v == 2:
                Pij[v, 2, 2] = -1.0
    return Pij


def _pow2_below(x):
    return 2.0 ** math.floor(math.log2(x))


def _new_geometry(geom, D, stage0, h, w):
    """-> (Pij [V, 4, 4] fp32, d0 [h * w] fp32) of one of NEW_GEOMS (module docstring)."""
    incre = incre_of(stage0)
    P = h * w
    H = float(np.float32((D // 2) * incre)) if stage0 else float(np.float32(0.00125))      # centre of the hypothesis range (stage 0: lim)
    jit = hashed((P,), 313, -1.5, 1.5).double()
    ys, xs = torch.arange(P) // w, torch.arange(P) % w
    if geom == "zero_over_zero":                            # only every fifth pixel is jittered: the others' hypothesis D // 2 is exactly H
        jit = torch.where((xs + 2 * ys) % 5 == 4, jit, torch.zeros_like(jit))
    d0 = (H + incre * jit).float()

    def lin(ax, ay, c, per_step):
        """Row of Pij with value ax x + ay y + c + per_step s, s = (hyp - H) / incre."""
        m3 = per_step / incre
        return [ax, ay, c - m3 * H, m3]

    r = 64.0 / D                                            # a sweep given per step at D = 64 covers the same texels at every D
    rows = []
    for v in range(V):
        if geom == "zoom_in_map":
            X = lin(6.0, 0.0, 2.0 + v, 0.25 * r * (1.0, -1.0, 0.5)[v])
            Y = lin(0.0, 6.0, 1.0, 0.08 * r * v)
            Z = lin(5.0 / w, 5.0 / h, 1.0, 0.0)
        elif geom == "wild_in_map":
            if v == 2:                                      # entirely behind the camera, and in the map
                X, Y, Z = lin(-1.0, 0.0, -0.4, -0.15 * r), lin(0.0, -1.0, -0.3, 0.02 * r), lin(-0.002, 0.0, -1.0, 0.0)
            else:
                zs, A, e1 = 0.05, 0.8 * D, 0.9
                Z = lin(-zs * A * 2 / w, 0.0, zs * A, zs) if v == 0 else lin(0.0, -zs * A * 2 / h, zs * A, zs)
                cx, cy = w / 2 - 0.37 - v, h / 2 - 0.37
                X = [cx * z + e for z, e in zip(Z, (e1 * zs, 0.0, e1 * zs * (0.3 - w / 2), 0.0))]
                Y = [cy * z + e for z, e in zip(Z, (0.0, e1 * zs, e1 * zs * (0.2 - h / 2), 0.0))]
        elif geom == "zero_over_zero":
            if v == 2:
                X, Y, Z = lin(1.0, 0.0, 0.3, 0.1 * r), lin(0.0, 1.0, 0.2, 0.0), lin(0.0, 0.0, 1.0, 0.0)
            else:
                cx, cy, g = _pow2_below(w / 2), _pow2_below(h / 2), _pow2_below(0.5 * incre)
                Z = [0.0, 0.0, -H, 1.0]
                X = [g, -g, -cx * H, cx] if v == 0 else [g, g, -cx * H + 1.5 * g, cx]
                Y = [0.0, 0.5 * g, -cy * H + 0.25 * g, cy] if v == 0 else [g, -2.0 * g, -cy * H, cy]
        elif geom == "border_graze":
            Z = lin(0.0, 0.0, 1.0, 0.0)
            if v == 0:
                X, Y = lin(0.01, 0.0, -0.9, 1.2 / D), lin(0.0, (h + 0.5) / max(h - 1, 1), -0.8, 0.0)
            elif v == 1:
                X, Y = lin(0.01, 0.0, w - 0.75, -1.2 / D), lin(0.0, 1.0, 0.3, 0.5 / D)
            else:
                X, Y = lin(0.01, 0.0, -1.5, 5.0 / D), lin(0.0, 0.02, h, -5.0 / D)
        else:
            raise ValueError(geom)
        rows.append([X, Y, Z, [0.0, 0.0, 0.0, 1.0]])
    return torch.tensor(rows, dtype=torch.float64).float(), d0


@functools.lru_cache(maxsize=None)
def lines_geometry(geom, D, stage0, h1, w1):
    """-> (fmaps [V + 1, C, h1, w1], Pij [V, 4, 4], d0 [h1 * w1]) fp32 on the CPU."""
    fm = hashed((1, V + 1, C, h1, w1), 311, -2, 2)[0]
    if geom in OLD_GEOMS:
        Pij = _old_pij(geom, stage0, h1, w1)
        d0 = hashed((h1 * w1,), 312, 0.0005, 0.002) if not stage0 else torch.zeros(h1 * w1)
    else:
        Pij, d0 = _new_geometry(geom, D, stage0, h1, w1)
    return fm, Pij, d0


def rows_of(fmaps):
    """What the kernels read (cer-mvs_amd/corr.py::fmaps_to_nhwc, without the border): -> (f1 [P, C], f2 [V, h, w, C]) = fmaps / 8."""
    nhwc = fmaps.permute(0, 2, 3, 1) * 0.125
    return nhwc[0].reshape(-1, nhwc.shape[-1]).contiguous(), nhwc[1:].contiguous()


# ------------------------------------------------------------------------------------------------ references, cached
@functools.lru_cache(maxsize=32)
def coords(geom, D, stage0, h, w, y0=0, rows=None):
    """``pc.cost_coords32`` of a case, or of its row slab y0 .. y0 + rows - 1."""
    _, Pij, d0 = lines_geometry(geom, D, stage0, h, w)
    rows = h - y0 if rows is None else rows
    return pc.cost_coords32(Pij, D, incre_of(stage0), d0[y0 * w:(y0 + rows) * w], stage0, rows, w, y0=y0)


@functools.lru_cache(maxsize=16)
def samples(geom, D, stage0, h, w, two_term=False, y0=0, rows=None):
    """``pc.cost_samples_ref64`` per view, [V, P, D] (V = 1 is its first view); the cache keeps the last few cases (a test walks through
    the builders and view counts of one case at a time) and, at the largest size, not the per-corner dots."""
    fm, _, _ = lines_geometry(geom, D, stage0, h, w)
    f1, f2 = rows_of(fm)
    rows = h - y0 if rows is None else rows
    S = pc.cost_samples_ref64(f1[y0 * w:(y0 + rows) * w], f2, coords(geom, D, stage0, h, w, y0, rows), f2_round=pc.cost_f2_two_term if two_term else None)
    if (h, w) == BIG:
        S.pop("dots")
    return S


def first_views(S, nv):
    return {k: t[:nv] for k, t in S.items()}


def floored(R):
    """The norm of rows ``R`` (``pc.cost_rows_ref64``) floored at the case's mean |ref| over the columns a builder writes."""
    m = R["level"] >= 0
    return R["norm"].clamp_min(float(R["ref"][:, m].abs().mean()))


# ------------------------------------------------------------------------------------------------ census
def epipole_inside(Pij, h, w):
    """Per view: does the reference epipole (A e ~ t, A = Pij[:3, :3], t = Pij[:3, 3]: csrc/cost_lines.hip::cost_lines_setup_kernel) lie
    inside the image?"""
    out = []
    for m in Pij.double().numpy():
        A, t = m[:3, :3], m[:3, 3]
        adj = np.linalg.det(A) * np.linalg.inv(A) if abs(np.linalg.det(A)) > 1e-300 else np.zeros((3, 3))
        e = adj @ t
        out.append(bool(abs(e[2]) > 1e-12 * (abs(e[0]) + abs(e[1]) + 1e-300) and 0 <= e[0] / e[2] <= w - 1 and 0 <= e[1] / e[2] <= h - 1))
    return out


def _widest_band(co, v, h, w):
    """Texels across the band of the widest 32-pixel tile of view v: tiles are straight 32-pixel runs of a row or of a column (the
    kernel's shear is not restated; both are taken, the narrower partition counts), the band's major axis is the coordinate with the larger
    extent, its width the extent of the other one around the least-squares line (slope limited to +-4, as the kernel's)."""
    u, t = co["u"][v].reshape(h, w, -1).astype(np.float64), co["t"][v].reshape(h, w, -1).astype(np.float64)
    use = co["ok"][v].reshape(h, w, -1) & (u >= -2) & (u <= w + 1) & (t >= -2) & (t <= h + 1)
    widest = []
    for axis in (0, 1):
        best = 0.0
        n_line, n_along = (h, w) if axis == 0 else (w, h)
        for j in range(n_line):
            for s in range(0, n_along, 32):
                sl = (j, slice(s, s + 32)) if axis == 0 else (slice(s, s + 32), j)
                m = use[sl]
                if m.sum() < 2:
                    continue
                a, b = u[sl][m], t[sl][m]
                if np.ptp(b) > np.ptp(a):
                    a, b = b, a
                var = a.var()
                slope = float(np.clip(((a - a.mean()) * (b - b.mean())).mean() / var, -4, 4)) if var > 1e-12 else 0.0
                best = max(best, float(np.ptp(b - slope * a)))
        widest.append(best)
    return min(widest)


@functools.lru_cache(maxsize=None)
def census(geom, D, stage0, h, w):
    """What a case samples, per view, from the restated coordinates -> list of V dicts: in_map (share of the samples with u in (-1, w) and
    t in (-1, h)), z_sign (share of the pixels whose Z changes sign over the hypotheses), in_map_pos / in_map_neg (share of the in-map
    samples with Z > 0 / Z < 0), not_ok (count), graze (count of samples with exactly one or two corners in the map), band (texels),
    epipole_inside, one_cell (every hypothesis of every pixel lands in one cell)."""
    _, Pij, _ = lines_geometry(geom, D, stage0, h, w)
    co = coords(geom, D, stage0, h, w)
    epi = epipole_inside(Pij, h, w)
    out = []
    for v in range(V):
        ok, u, t, Z, iu, iw = (co[k][v] for k in ("ok", "u", "t", "Z", "iu", "iw"))
        inm = ok & (u > -1) & (u < w) & (t > -1) & (t < h)
        ncorner = sum((ok & (iu + dx >= 0) & (iu + dx < w) & (iw + dy >= 0) & (iw + dy < h)).astype(np.int32) for dy, dx in pc.CORNERS)
        n_in = max(int(inm.sum()), 1)
        out.append(dict(in_map=float(inm.mean()), z_sign=float(((Z.min(1) < 0) & (Z.max(1) > 0)).mean()),
                        in_map_pos=float((inm & (Z > 0)).sum() / n_in), in_map_neg=float((inm & (Z < 0)).sum() / n_in),
                        not_ok=int((~ok).sum()), graze=int(((ncorner == 1) | (ncorner == 2)).sum()), band=_widest_band(co, v, h, w),
                        epipole_inside=epi[v], one_cell=bool((iu == iu[:, :1]).all() and (iw == iw[:, :1]).all())))
    return out
