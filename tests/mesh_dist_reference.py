"""Exact point-to-mesh distance restated in numpy (the contract is cer_mvs.h's, "Mesh distance") with other means than
csrc/mesh_dist.hip's: a brute force over ALL faces where the kernel walks a grid, ``np.select`` where it branches, ``argmin`` on (dist2,
index) where it keeps a running best; the per-face cell counts and the pair list as loops over boxes; a search that visits only the faces
whose box of cells lies within the padded gap of the query; and the same closest point in exact rational arithmetic."""
import math
from fractions import Fraction

import numpy as np

import mesh_sample_reference as R

INFO_KEYS = ("cell", "pairs", "faces_indexed", "cells")
MAX_CELLS = 4096
COORD_LIMIT = 1 << 20
B = COORD_LIMIT - 1
GRID_EPS = 1e-6


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def closest_on_triangles(a, b, c, p):
    """a, b, c, p: float64 [..., 3], broadcast against each other -> (dist2 [...], q [..., 3], region [...] in 1 .. 7).  The select form:
    every region's candidate is computed, the first region that holds picks."""
    with np.errstate(all="ignore"):
        ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
        region = np.select(conds, [1, 2, 3, 4, 5, 6], default=7)
        w6 = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = (va + vb) + vc
        zero = np.zeros_like(d1)
        v = np.select([region == 3, region == 6, region == 7], [d1 / (d1 - d3), 1.0 - w6, vb / den], default=zero)
        w = np.select([region == 5, region == 6, region == 7], [d2 / (d2 - d6), w6, vc / den], default=zero)
        e = (a + v[..., None] * ab) + w[..., None] * ac
        r = region[..., None]
        q = np.where(r == 1, a, np.where(r == 2, b, np.where(r == 4, c, e)))
        d = q - p
        dist2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return dist2, q, region


def indexed_faces(vertices, faces):
    """the faces that are entered in the index: those that ``face_areas`` gives an area above 0"""
    return R.face_areas(vertices, faces) > 0.0


def limit_of(max_dist):
    m = np.float64(np.float32(max_dist))
    return m * m


def brute(vertices, faces, queries, max_dist, chunk=128, subset=None):
    """-> (dist float32 [m], face int32 [m], closest float32 [m, 3]): every query against every indexed face (``subset(i0, i1)`` -> bool
    [rows, nf] narrows that, for the index search below), winner = argmin on (dist2, index) among dist2 <= double(max_dist)^2"""
    v, f = R.as_vertices(vertices), R.as_faces(faces)
    qs = np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
    m = len(qs)
    dist, face, near = np.full(m, np.inf, np.float32), np.full(m, -1, np.int32), np.full((m, 3), np.nan, np.float32)
    rows = np.flatnonzero(indexed_faces(v, f))
    if m == 0 or len(rows) == 0:
        return dist, face, near
    p64 = v.astype(np.float64)
    a, b, c = p64[f[rows, 0]][None], p64[f[rows, 1]][None], p64[f[rows, 2]][None]
    limit = limit_of(max_dist)
    for i0 in range(0, m, chunk):
        q = qs[i0:i0 + chunk].astype(np.float64)
        d2, pt, _ = closest_on_triangles(a, b, c, q[:, None, :])
        ok = (d2 <= limit) & np.isfinite(qs[i0:i0 + chunk]).all(1)[:, None]                    # (false for a NaN)
        if subset is not None:
            ok &= subset(i0, i0 + len(q))[:, rows]
        key = np.where(ok, d2, np.inf)
        j = np.argmin(key, axis=1)                                                             # the first minimum: the lowest face index
        k = np.arange(len(q))
        found = ok[k, j]
        with np.errstate(all="ignore"):
            dist[i0:i0 + chunk] = np.where(found, np.sqrt(d2[k, j]).astype(np.float32), np.float32(np.inf))
        face[i0:i0 + chunk] = np.where(found, rows[j], -1)
        near[i0:i0 + chunk] = np.where(found[:, None], pt[k, j].astype(np.float32), np.float32(np.nan))
    return dist, face, near


# ---------------------------------------------------------------- the index: frame, boxes, counts and pairs
def origin_of(vertices, faces):
    """per-axis minimum of the vertices that indexed faces use, in fp64; None for a mesh without an indexed face"""
    v, f = R.as_vertices(vertices), R.as_faces(faces)
    rows = indexed_faces(v, f)
    if not rows.any():
        return None
    return v[f[rows].reshape(-1)].min(0).astype(np.float64)


def boxes(vertices, faces, cell, origin=None):
    """-> (origin, lo int64 [nf, 3], hi int64 [nf, 3], indexed bool [nf]): the box of cells of every face, floor((double(x) - origin) /
    cell) of its smallest and largest corner coordinate; zeros for a face that is left out"""
    v, f = R.as_vertices(vertices), R.as_faces(faces)
    rows = indexed_faces(v, f)
    origin = origin_of(v, f) if origin is None else np.asarray(origin, np.float64)
    lo, hi = np.zeros((len(f), 3), np.float64), np.zeros((len(f), 3), np.float64)
    if rows.any():
        corners = v[f[rows]]                                                                   # [k, 3 corners, 3 axes] float32
        lo[rows] = np.floor((corners.min(1).astype(np.float64) - origin) / np.float64(cell))
        hi[rows] = np.floor((corners.max(1).astype(np.float64) - origin) / np.float64(cell))
    return origin, lo, hi, rows


def cell_counts(vertices, faces, cell, origin=None):
    """-> (counts int64 [nf], beyond, large): the cells per face (0 for a face that is left out, that leaves the key range or that exceeds
    the cap), whether a face leaves the key range, whether one exceeds the cap of MAX_CELLS cells"""
    _, lo, hi, rows = boxes(vertices, faces, cell, origin)
    outside = rows & ((np.abs(lo) > B) | (np.abs(hi) > B)).any(1)
    ext = np.where((rows & ~outside)[:, None], hi - lo + 1, 0)
    counts = [int(e[0]) * int(e[1]) * int(e[2]) for e in ext]                                  # Python integers
    large = [n > MAX_CELLS for n in counts]
    return np.array([0 if big else n for n, big in zip(counts, large)], np.int64), bool(outside.any()), bool(any(large))


def key_of(x, y, z):
    return ((int(z) + B) << 42) | ((int(y) + B) << 21) | (int(x) + B)


def pairs(vertices, faces, cell, origin=None):
    """-> (keys int64 [npairs], ids int32 [npairs]) in the order they are written: face by face, z-major, then y, then x"""
    _, lo, hi, _ = boxes(vertices, faces, cell, origin)
    counts, beyond, large = cell_counts(vertices, faces, cell, origin)
    assert not beyond and not large
    keys, ids = [], []
    for face in np.flatnonzero(counts):
        (x0, y0, z0), (x1, y1, z1) = lo[face].astype(np.int64), hi[face].astype(np.int64)
        for z in range(z0, z1 + 1):
            for y in range(y0, y1 + 1):
                for x in range(x0, x1 + 1):
                    keys.append(key_of(x, y, z))
                    ids.append(face)
    return np.array(keys, np.int64), np.array(ids, np.int32)


def info_of(vertices, faces, cell):
    keys, _ = pairs(vertices, faces, cell)
    return dict(cell=float(cell), pairs=len(keys), faces_indexed=int(indexed_faces(vertices, faces).sum()), cells=len(np.unique(keys)))


def default_cell(vertices, faces, max_dist=None):
    """max(4 * sqrt(area / faces with weight), max_dist / 32) on the sampling's exact integer table"""
    info = R.info_of(vertices, faces, 0)
    cell = 4.0 * math.sqrt(info["area"] / info["faces_with_weight"]) if info["faces_with_weight"] else 0.0
    if max_dist is not None and math.isfinite(float(np.float32(max_dist))):
        cell = max(cell, float(np.float32(max_dist)) / 32)
    return cell if cell > 0.0 and math.isfinite(cell) else 1.0


def index_search(vertices, faces, queries, max_dist, cell):
    """``brute`` over only the faces that the grid can show a query: those with a cell of their box within the padded gap - per axis the
    gap, in cells, between the query's u = (double(x) - origin) / cell and the box [lo, hi + 1), less GRID_EPS and not below 0, times the
    cell; squared and summed; not beyond double(max_dist)^2.  What the walk may skip is only ever outside this set."""
    v, f = R.as_vertices(vertices), R.as_faces(faces)
    origin, lo, hi, rows = boxes(v, f, cell)
    qs = np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
    if origin is None:
        return brute(v, f, qs, max_dist)
    limit = limit_of(max_dist)
    with np.errstate(all="ignore"):
        u = (qs.astype(np.float64) - origin) / np.float64(cell)

    def subset(i0, i1):
        with np.errstate(all="ignore"):
            uq = u[i0:i1, None, :]
            gap = np.maximum(np.maximum(lo[None] - uq - GRID_EPS, uq - (hi[None] + 1.0) - GRID_EPS), 0.0) * np.float64(cell)
            g2 = (gap * gap).sum(2)
        return rows[None] & (g2 <= limit)
    return brute(v, f, qs, max_dist, subset=subset)


# ---------------------------------------------------------------- exact
def exact_dist2(a, b, c, p):
    """the same regions in rational arithmetic on exact inputs (sequences of three ints, Fractions or floats) -> (dist2, q, region)"""
    a, b, c, p = ([Fraction(x) for x in t] for t in (a, b, c, p))

    def sub(x, y):
        return [s - t for s, t in zip(x, y)]

    def dot(x, y):
        return sum(s * t for s, t in zip(x, y))
    ab, ac, ap, bp, cp = sub(b, a), sub(c, a), sub(p, a), sub(p, b), sub(p, c)
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    if d1 <= 0 and d2 <= 0:
        region, q = 1, a
    elif d3 >= 0 and d4 <= d3:
        region, q = 2, b
    elif vc <= 0 and d1 >= 0 and d3 <= 0:
        region, v, w = 3, d1 / (d1 - d3), Fraction(0)
    elif d6 >= 0 and d5 <= d6:
        region, q = 4, c
    elif vb <= 0 and d2 >= 0 and d6 <= 0:
        region, v, w = 5, Fraction(0), d2 / (d2 - d6)
    elif va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0:
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        region, v = 6, 1 - w
    else:
        den = va + vb + vc
        region, v, w = 7, vb / den, vc / den
    if region in (3, 5, 6, 7):
        q = [s + v * t + w * r for s, t, r in zip(a, ab, ac)]
    r = sub(q, p)
    return dot(r, r), q, region
