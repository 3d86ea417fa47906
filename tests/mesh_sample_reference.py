"""Mesh surface sampling restated in numpy and Python integers (the contract is cer_mvs.h's, "Mesh surface sampling"): areas,
integer weights, Philox4x32-10, the face pick, the fold, positions, normals, colours and the even sampling - with other means than
csrc/mesh_sample.hip's: ``np.searchsorted`` where the kernel bisects, Python's big integers where it takes the high half of a 128-bit
product, ``np.cumsum`` where the caller scans on the device, and the sequential greedy loop of the thinning tests for ``sample_mesh_even``."""
import math

import numpy as np

INFO_KEYS = ("n", "area", "faces_with_weight", "shift")
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
TWO32 = 1 << 32


def as_vertices(vertices):
    return np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)


def as_faces(faces):
    return np.ascontiguousarray(faces, np.int32).reshape(-1, 3)


# ---------------------------------------------------------------- areas and weights
def _valid(v, f):
    """faces whose indices are in range and distinct"""
    nv = len(v)
    inside = ((f >= 0) & (f < nv)).all(1)
    return inside & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])


def _cross(v, f, rows):
    """(nx, ny, nz) of the faces ``rows`` in fp64, every product and difference rounded on its own"""
    p = v.astype(np.float64)
    a, b, c = p[f[rows, 0]], p[f[rows, 1]], p[f[rows, 2]]
    e1, e2 = b - a, c - a
    with np.errstate(all="ignore"):
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return nx, ny, nz


def face_areas(vertices, faces):
    v, f = as_vertices(vertices), as_faces(faces)
    out = np.zeros(len(f), np.float64)
    ok = _valid(v, f)
    rows = np.flatnonzero(ok)
    rows = rows[np.isfinite(v[f[rows]].reshape(len(rows), 9)).all(1)]
    nx, ny, nz = _cross(v, f, rows)
    with np.errstate(all="ignore"):
        out[rows] = 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)      # numpy's sqrt is correctly rounded
    return out


def shift_of(amax):
    return 32 - math.frexp(float(amax))[1]


def face_weights(areas, shift):
    """floor(areas * 2^shift) as Python integers, held to what the kernel writes: 0 for a NaN, a negative value or 2^63 and beyond"""
    out = np.zeros(len(areas), np.int64)
    for i, a in enumerate(np.asarray(areas, np.float64).tolist()):
        if a == a and a >= 0.0 and a != math.inf:
            w = math.floor(math.ldexp(a, shift)) if a else 0
            out[i] = w if w < (1 << 63) else 0
    return out


def table(vertices, faces):
    """-> (cum int64 [nf], W, shift, areas): what ``sample_mesh`` builds before it draws; W = 0 and shift = 0 for a mesh without area"""
    areas = face_areas(vertices, faces)
    amax = float(areas.max()) if len(areas) else 0.0
    if not amax > 0.0:
        return np.zeros(len(areas), np.int64), 0, 0, areas
    shift = shift_of(amax)
    weights = face_weights(areas, shift)
    total = sum(int(w) for w in weights)                      # Python integers: exact
    cum = np.cumsum(weights)
    assert int(cum[-1]) == total < (1 << 63)
    return cum, total, shift, areas


def info_of(vertices, faces, n):
    cum, W, shift, _ = table(vertices, faces)
    return dict(n=int(n), area=math.ldexp(float(W), -shift), faces_with_weight=int((np.diff(cum, prepend=0) > 0).sum()), shift=shift)


# ---------------------------------------------------------------- Philox4x32-10
def philox(counter, key):
    """one block of Philox4x32-10 in Python integers: counter (c0 .. c3), key (k0, k1) -> (x0 .. x3)"""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def philox_words(seed, offset, n):
    """uint32 [n, 4]: the words of the samples offset .. offset + n - 1 (the index wraps at 2^64), ten vectorised rounds in uint64"""
    k = (np.arange(n, dtype=np.uint64) + np.uint64(offset % (1 << 64)))        # (uint64 addition wraps)
    c = [k & np.uint64(MASK32), k >> np.uint64(32), np.zeros(n, np.uint64), np.zeros(n, np.uint64)]
    k0, k1 = seed & MASK32, (seed >> 32) & MASK32
    m32 = np.uint64(MASK32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                       # 32 x 32 bits: fits 64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return np.stack(c, 1).astype(np.uint32)


# ---------------------------------------------------------------- samples
def pick_faces(cum, W, words):
    """t = (r * W) >> 64 in Python integers, then the number of prefix sums <= t: the smallest index with cum[f] > t"""
    x = np.asarray(words, np.uint32).reshape(-1, 4)
    t = np.array([((int(x0) * TWO32 + int(x1)) * W) >> 64 for x0, x1 in zip(x[:, 0].tolist(), x[:, 1].tolist())], np.int64)
    return np.minimum(np.searchsorted(cum, t, side="right"), len(cum) - 1).astype(np.int32)


def barycentric(words):
    """-> (u, v, w) float64 [n]: the fold of the unit square onto the triangle"""
    x = np.asarray(words, np.uint32).reshape(-1, 4)
    a, b = x[:, 2].astype(np.int64), x[:, 3].astype(np.int64)
    fold = a + b >= TWO32
    a, b = np.where(fold, TWO32 - 1 - a, a), np.where(fold, TWO32 - 1 - b, b)
    u, v = (a.astype(np.float64) + 0.5) * 2.0 ** -32, (b.astype(np.float64) + 0.5) * 2.0 ** -32
    return u, v, (1.0 - u) - v


def sample_with(vertices, faces, cum, W, words, normals=False, colors=None, uv=False):
    """the samples of ``words`` under a given table -> (points, face, normals | None, colors | None, uv | None)"""
    v, f = as_vertices(vertices), as_faces(faces)
    x = np.asarray(words, np.uint32).reshape(-1, 4)
    n = len(x)
    if n == 0:
        return (np.zeros((0, 3), np.float32), np.zeros(0, np.int32), np.zeros((0, 3), np.float32) if normals else None,
                None if colors is None else np.zeros((0, 3), np.uint8), np.zeros((0, 2), np.float64) if uv else None)
    face = pick_faces(cum, W, x)
    bu, bv, bw = barycentric(x)
    ok = _valid(v, f)[face]
    rows = face[ok]
    p = v.astype(np.float64)
    points = np.full((n, 3), np.nan, np.float32)
    A, B, C = p[f[rows, 0]], p[f[rows, 1]], p[f[rows, 2]]
    w_, u_, v_ = bw[ok, None], bu[ok, None], bv[ok, None]
    with np.errstate(all="ignore"):
        points[ok] = ((w_ * A + u_ * B) + v_ * C).astype(np.float32)
    out_n = out_c = None
    if normals:
        out_n = np.full((n, 3), np.nan, np.float32)
        nx, ny, nz = _cross(v, f, rows)
        with np.errstate(all="ignore"):
            length = np.sqrt((nx * nx + ny * ny) + nz * nz)
            out_n[ok] = np.stack([nx / length, ny / length, nz / length], 1).astype(np.float32)
    if colors is not None:
        col = np.asarray(colors, np.uint8).astype(np.float64)
        out_c = np.zeros((n, 3), np.uint8)
        mixed = np.floor(((w_ * col[f[rows, 0]] + u_ * col[f[rows, 1]]) + v_ * col[f[rows, 2]]) + 0.5)
        out_c[ok] = np.minimum(mixed, 255.0).astype(np.uint8)
    return points, face, out_n, out_c, (np.stack([bu, bv], 1) if uv else None)


def sample(vertices, faces, n=None, seed=0, offset=0, words=None, normals=False, colors=None, uv=False):
    """``mesh.sample_mesh`` restated (n or words; a density is the caller's arithmetic) -> ((points, face, normals, colors, uv), info)"""
    cum, W, shift, _ = table(vertices, faces)
    x = philox_words(seed, offset, n) if words is None else np.asarray(words, np.uint32).reshape(-1, 4)
    if len(x) and W == 0:
        raise ValueError("no area to sample")
    return sample_with(vertices, faces, cum, W, x, normals, colors, uv), info_of(vertices, faces, len(x))


def count_for(area, density):
    return int(math.ceil(area * density))


# ---------------------------------------------------------------- even sampling
def near(points, radius):
    """bool [n, n]: d2(i, j) <= double(float32(radius))^2, d2 = (dx*dx + dy*dy) + dz*dz in fp64 (``radius_thin``'s contract)"""
    P = np.asarray(points, np.float32).astype(np.float64)
    limit = np.float64(np.float32(radius)) * np.float64(np.float32(radius))
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (P[None, :, k] - P[:, None, k] for k in range(3))
        return ((dx * dx + dy * dy) + dz * dz) <= limit


def greedy(points, radius):
    """the sequential loop in index order: a point that is still in the set stays and removes every point within the radius"""
    nb, alive, kept = near(points, radius), np.isfinite(np.asarray(points, np.float32)).all(1), []
    for i in range(len(alive)):
        if alive[i]:
            kept.append(i)
            alive &= ~nb[i]
    return np.asarray(kept, np.int64)


def drawn_for(area, spacing, oversample=8.0):
    return int(math.ceil(oversample * area / (float(spacing) * float(spacing))))


def sample_even(vertices, faces, spacing, oversample=8.0, seed=0, normals=False, colors=None, thin=greedy):
    """``mesh.sample_mesh_even`` restated -> ((points, face, normals, colors), kept indices, drawn)"""
    n0 = drawn_for(info_of(vertices, faces, 0)["area"], spacing, oversample)
    (p, face, nrm, col, _), _ = sample(vertices, faces, n=n0, seed=seed, normals=normals, colors=colors)
    kept = thin(p, spacing)
    return (p[kept], face[kept], None if nrm is None else nrm[kept], None if col is None else col[kept]), kept, n0


# ---------------------------------------------------------------- fixtures
def random_colors(nv, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (nv, 3), dtype=np.uint8)


def random_mesh(nf, seed, zero_runs=True):
    """a small random soup of nf faces over nf + 4 vertices; with ``zero_runs`` (nf >= 5) faces without weight at the start, at the end and
    in a run in the middle - a repeated index, a sliver far below 2^-32 of the largest and collapsed corners"""
    rng = np.random.default_rng(seed)
    nv = nf + 4
    v = rng.uniform(-1.0, 1.0, (nv, 3)).astype(np.float32)
    f = np.stack([rng.permutation(nv)[:3] for _ in range(nf)]).astype(np.int32)
    if zero_runs and nf >= 5:
        dead = sorted({0, nf - 1} | set(range(nf // 2, nf // 2 + max(1, nf // 8))))
        for j, i in enumerate(dead):
            if j % 3 == 0:
                f[i, 2] = f[i, 0]                             # a repeated index
            elif j % 3 == 1:
                f[i] = (nv, 0, 1)                             # an index out of range
            else:
                f[i, 1] = -1
    return v, f


def in_triangle(points, vertices, faces, face):
    """-> (the largest distance from the face's plane, the largest distance by which a sample lies beyond an edge of its face within that
    plane), both relative to the largest coordinate of the face, in fp64"""
    p = np.asarray(points, np.float64)
    v = as_vertices(vertices).astype(np.float64)
    f = as_faces(faces)[face]
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    nrm = np.cross(b - a, c - a)
    unit = nrm / np.linalg.norm(nrm, axis=1)[:, None]
    size = np.maximum(np.abs(a).max(1), np.maximum(np.abs(b).max(1), np.abs(c).max(1)))
    height = ((p - a) * unit).sum(1)
    q = p - height[:, None] * unit

    def beyond(s, e):                                         # positive on the outer side of the directed edge s -> e
        return -(np.cross(e - s, q - s) * unit).sum(1) / np.linalg.norm(e - s, axis=1)
    out = np.maximum(beyond(a, b), np.maximum(beyond(b, c), beyond(c, a)))
    return float((np.abs(height) / size).max()), float((out / size).max())
