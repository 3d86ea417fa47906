"""numpy restatement of the mesh simplification (csrc/mesh.hip, cer-mvs_amd/mesh.py simplify_vertex_clustering), written from
the contract in include/cer_mvs.h ("Mesh simplification") with OTHER algorithms than the device's: np.unique on the cell keys instead of a
sort and a head scan, unbuffered np.add.at in member order instead of one thread per cluster, a Python dictionary for the duplicate faces
instead of two sorts and a head pass, and a boolean scatter with a cumulative sum for the selection.  Every fp64 expression carries the
contract's association; no np.sum (its pairwise order is not the contract's).  Plus the cases the tests share."""
import numpy as np

import mesh_reference as M

KEY_B = (1 << 20) - 1                                        # cer_mvs.h CER_GRID_COORD_LIMIT - 1
REPRESENTATIVES = ("quadric", "mean")


def as_vertices(vertices):
    return np.ascontiguousarray(np.asarray(vertices, dtype=np.float32).reshape(-1, 3))


def as_faces(faces):
    return np.ascontiguousarray(np.asarray(faces, dtype=np.int32).reshape(-1, 3))


def clusters(vertices, cell):
    """(cluster int64 [nv]: the rank of every vertex's cell key among the distinct keys, -1 for a non-finite vertex; cells int64 [nc, 3]: the
    cell coordinates of every cluster; origin float64 [3])"""
    v = as_vertices(vertices).astype(np.float64)
    finite = np.isfinite(v).all(1)
    cluster = np.full(len(v), -1, dtype=np.int64)
    if not finite.any():
        return cluster, np.zeros((0, 3), np.int64), np.zeros(3)
    origin = v[finite].min(0)
    c = np.floor((v[finite] - origin) / float(cell)).astype(np.int64)
    if c.max() > KEY_B:
        raise ValueError("more than 2^20 cells along an axis")
    keys = ((c[:, 2] + KEY_B) << 42) | ((c[:, 1] + KEY_B) << 21) | (c[:, 0] + KEY_B)
    distinct, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    cluster[finite] = inverse.reshape(-1)
    return cluster, c[first], origin


def quadric_systems(vertices, faces, cell):
    """What the contract sums per cluster, in its order: (cluster, cells, origin, count int64 [nc], mean float64 [nc, 3], base [nc, 3], M [nc, 6]
    as (xx, xy, xz, yy, yz, zz), q [nc, 3])"""
    v32, f = as_vertices(vertices), as_faces(faces)
    v = v32.astype(np.float64)
    cluster, cells, origin = clusters(v32, cell)
    nc = len(cells)
    members = np.flatnonzero(cluster >= 0)                    # ascending vertex index: within a cluster, member order
    count = np.zeros(nc, np.int64)
    np.add.at(count, cluster[members], 1)
    s = np.zeros((nc, 3))
    for a in range(3):
        np.add.at(s[:, a], cluster[members], v[members, a])
    with np.errstate(all="ignore"):
        mean = s / count[:, None].astype(np.float64)
    base = origin + (cells.astype(np.float64) + 0.5) * float(cell)
    # the corner entries in (vertex ascending, corner id ascending) order: within a cluster that is member order, then the member's corners
    flat = f.reshape(-1).astype(np.int64)
    entries = np.argsort(flat, kind="stable")
    entries = entries[cluster[flat[entries]] >= 0]
    owner = cluster[flat[entries]]
    tri = f[entries // 3].astype(np.int64)
    A, B, C = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    Mq, q = np.zeros((nc, 6)), np.zeros((nc, 3))
    with np.errstate(all="ignore"):
        U, W = B - A, C - A
        nx = U[:, 1] * W[:, 2] - U[:, 2] * W[:, 1]
        ny = U[:, 2] * W[:, 0] - U[:, 0] * W[:, 2]
        nz = U[:, 0] * W[:, 1] - U[:, 1] * W[:, 0]
        rel = A - base[owner]
        d = (nx * rel[:, 0] + ny * rel[:, 1]) + nz * rel[:, 2]
        for k, prod in enumerate((nx * nx, nx * ny, nx * nz, ny * ny, ny * nz, nz * nz)):
            np.add.at(Mq[:, k], owner, prod)
        for k, prod in enumerate((nx * d, ny * d, nz * d)):
            np.add.at(q[:, k], owner, prod)
    return cluster, cells, origin, count, mean, base, Mq, q


def regularised(Mq, q, mean, base, regularisation):
    """(lam [nc], the symmetric matrices M + lam I as [nc, 3, 3], the right-hand sides q + lam (mean - base) [nc, 3])"""
    with np.errstate(all="ignore"):
        lam = (float(regularisation) * ((Mq[:, 0] + Mq[:, 3]) + Mq[:, 5])) / 3.0
        a, dd, ff = Mq[:, 0] + lam, Mq[:, 3] + lam, Mq[:, 5] + lam
        rhs = q + lam[:, None] * (mean - base)
    mat = np.stack([np.stack([a, Mq[:, 1], Mq[:, 2]], 1), np.stack([Mq[:, 1], dd, Mq[:, 4]], 1), np.stack([Mq[:, 2], Mq[:, 4], ff], 1)], 1)
    return lam, mat, rhs


def cramer(mat, rhs):
    """(det [nc], x [nc, 3]) by the contract's cofactors"""
    a, b, c, dd, e, ff = mat[:, 0, 0], mat[:, 0, 1], mat[:, 0, 2], mat[:, 1, 1], mat[:, 1, 2], mat[:, 2, 2]
    tx, ty, tz = rhs[:, 0], rhs[:, 1], rhs[:, 2]
    with np.errstate(all="ignore"):
        c00 = dd * ff - e * e
        c01 = c * e - b * ff
        c02 = b * e - c * dd
        c11 = a * ff - c * c
        c12 = b * c - a * e
        c22 = a * dd - b * b
        det = (a * c00 + b * c01) + c * c02
        x = ((c00 * tx + c01 * ty) + c02 * tz) / det
        y = ((c01 * tx + c11 * ty) + c12 * tz) / det
        z = ((c02 * tx + c12 * ty) + c22 * tz) / det
    return det, np.stack([x, y, z], 1)


def representatives(vertices, faces, cell, representative="quadric", regularisation=1e-3):
    """(cluster, reps float32 [nc, 3], took bool [nc], parts): ``parts`` holds the fp64 pieces for the tests that look inside"""
    assert representative in REPRESENTATIVES
    cluster, cells, origin, count, mean, base, Mq, q = quadric_systems(vertices, faces if representative == "quadric" else np.zeros((0, 3), np.int32), cell)
    took = np.zeros(len(cells), dtype=bool)
    rep = mean.copy()
    parts = dict(cells=cells, origin=origin, count=count, mean=mean, base=base)
    if representative == "quadric":
        lam, mat, rhs = regularised(Mq, q, mean, base, regularisation)
        det, x = cramer(mat, rhs)
        with np.errstate(all="ignore"):
            took = (lam > 0.0) & (det > 0.0) & np.isfinite(det) & np.isfinite(x).all(1) & (np.abs(x) <= float(cell) / 2.0).all(1)
            rep[took] = (base + x)[took]
        parts.update(lam=lam, mat=mat, rhs=rhs, det=det, x=x)
    with np.errstate(all="ignore"):
        return cluster, rep.astype(np.float32), took, parts


def simplify(vertices, faces, cell, representative="quadric", regularisation=1e-3, colors=None):
    """((vertices', faces', cluster int32 [nv], colors' | None), info)"""
    v, f = as_vertices(vertices), as_faces(faces)
    nv, nf = len(v), len(f)
    cl, reps, took, parts = representatives(v, f, cell, representative, regularisation)
    nc = len(reps)
    rep_colors = None
    if colors is not None:
        col = np.asarray(colors, dtype=np.uint8).reshape(nv, 3).astype(np.int64)
        members = np.flatnonzero(cl >= 0)
        total = np.zeros((nc, 3), np.int64)
        for a in range(3):
            np.add.at(total[:, a], cl[members], col[members, a])
        rep_colors = (total // parts["count"][:, None]).astype(np.uint8)
    # faces: the cluster triple, rotated to its smallest id; the first of every distinct triple
    seen, kept, n_valid = {}, [], 0
    for i, (a, b, c) in enumerate(cl[f.astype(np.int64)].reshape(-1, 3).tolist()):
        if min(a, b, c) < 0 or a == b or b == c or a == c:
            continue
        n_valid += 1
        t = (a, b, c)
        k = t.index(min(t))
        t = t[k:] + t[:k]
        if t not in seen:
            seen[t] = i
            kept.append(t)
    kept = np.array(kept, dtype=np.int64).reshape(-1, 3)
    used = np.zeros(nc, dtype=bool)
    used[kept.reshape(-1)] = True
    new = np.cumsum(used) - 1
    out_cluster = np.where((cl >= 0) & used[np.maximum(cl, 0)], new[np.maximum(cl, 0)], -1).astype(np.int32) if nc else np.full(nv, -1, np.int32)
    info = dict(clusters=nc, degenerate_faces=nf - n_valid, duplicate_faces=n_valid - len(kept), dropped_clusters=nc - int(used.sum()),
                quadric=int(took.sum()))
    return (reps[used], new[kept].astype(np.int32).reshape(-1, 3), out_cluster, None if rep_colors is None else rep_colors[used]), info


# ---------------------------------------------------------------- checks of a result
def up_to_rotation(faces):
    """the set of faces as tuples rotated to their smallest index"""
    out = set()
    for t in as_faces(faces).tolist():
        k = t.index(min(t))
        out.add(tuple(t[k:] + t[:k]))
    return out


def guarantees(vertices, faces):
    """(distinct indices per face, no two faces equal up to rotation, every vertex referenced)"""
    f = as_faces(faces)
    distinct = bool(((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])).all())
    referenced = np.zeros(len(vertices), dtype=bool)
    referenced[f.reshape(-1)] = True
    return distinct, len(up_to_rotation(f)) == len(f), bool(referenced.all())


def closed(faces, nv):
    """every directed edge has its reverse (mesh_reference.edge_stats' second figure; an edge may appear more than once)"""
    return M.edge_stats(as_faces(faces), nv)[1] if len(faces) else True


# ---------------------------------------------------------------- cases
F32 = np.float32
NAN = float("nan")
QUAD = [[0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [0.0, 1.5, 0.0], [1.5, 1.5, 0.0]]          # at cell 1: clusters 0, 1, 2, 3 in this order


def half(a, b):
    """the mean representative of two members, per axis (float32 in, fp64 sum, one division, one rounding)"""
    return [float(F32((float(F32(x)) + float(F32(y))) / 2.0)) for x, y in zip(a, b)]


def hand_made():
    """name -> (vertices, faces, cell, the expected (vertices', faces', cluster) and info with the "mean" representative, written out by hand)"""
    B2 = [1.75, 0.25, 0.0]                                    # a second member of cluster 1
    tri = [[0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [0.0, 1.5, 0.0]]
    return {
        "an empty mesh": ([], [], 1.0, ([], [], []), dict(clusters=0, degenerate_faces=0, duplicate_faces=0, dropped_clusters=0, quadric=0)),
        "one triangle inside one cell": ([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [0.0, 0.5, 0.0]], [[0, 1, 2]], 1.0, ([], [], [-1, -1, -1]),
                                         dict(clusters=1, degenerate_faces=1, duplicate_faces=0, dropped_clusters=1, quadric=0)),
        "two triangles in four cells": (QUAD, [[0, 1, 2], [2, 1, 3]], 1.0, (QUAD, [[0, 1, 2], [1, 3, 2]], [0, 1, 2, 3]),
                                        dict(clusters=4, degenerate_faces=0, duplicate_faces=0, dropped_clusters=0, quadric=0)),
        "a fan that collapses to a duplicate pair": (tri + [B2], [[0, 3, 2], [0, 1, 3], [1, 2, 0]], 1.0,
                                                     ([tri[0], half(tri[1], B2), tri[2]], [[0, 1, 2]], [0, 1, 2, 1]),
                                                     dict(clusters=3, degenerate_faces=1, duplicate_faces=1, dropped_clusters=0, quadric=0)),
        "the pair with opposite orientation": (tri + [B2], [[0, 3, 2], [2, 1, 0]], 1.0,
                                               ([tri[0], half(tri[1], B2), tri[2]], [[0, 1, 2], [0, 2, 1]], [0, 1, 2, 1]),
                                               dict(clusters=3, degenerate_faces=0, duplicate_faces=0, dropped_clusters=0, quadric=0)),
        "a NaN vertex": (QUAD + [[NAN, 0.5, 0.5]], [[0, 1, 2], [1, 4, 3], [2, 1, 3]], 1.0, (QUAD, [[0, 1, 2], [1, 3, 2]], [0, 1, 2, 3, -1]),
                         dict(clusters=4, degenerate_faces=1, duplicate_faces=0, dropped_clusters=0, quadric=0)),
        "a face with a repeated index": (QUAD, [[0, 1, 1], [3, 2, 1], [2, 2, 2]], 1.0, (QUAD[1:], [[0, 2, 1]], [-1, 0, 1, 2]),
                                         dict(clusters=4, degenerate_faces=2, duplicate_faces=0, dropped_clusters=1, quadric=0)),
        "an unreferenced vertex": (QUAD + [[3.5, 3.5, 0.0]], [[0, 1, 2], [2, 1, 3]], 1.0, (QUAD, [[0, 1, 2], [1, 3, 2]], [0, 1, 2, 3, -1]),
                                   dict(clusters=5, degenerate_faces=0, duplicate_faces=0, dropped_clusters=1, quadric=0)),
    }


def sphere_mesh(n=12, r=4.2):
    """the analytic sphere mesh of mesh_reference: (vertices, faces, centre)"""
    tsdf, weight, grid, centre = M.sphere_field(n, r)
    v, f = M.extract_mesh(tsdf, weight, grid)
    return v, f, centre


def sphere_distances(vertices, centre, radius):
    """|distance to the centre - radius| per vertex, fp64"""
    return np.abs(np.linalg.norm(np.asarray(vertices, np.float64) - np.asarray(centre, np.float64), axis=1) - radius)


def renumbered(vertices, faces, seed):
    """the same mesh with its vertices renumbered by a seeded permutation and its faces shuffled: (vertices', faces', new index of every old
    vertex)"""
    rng = np.random.default_rng(seed)
    v, f = as_vertices(vertices), as_faces(faces)
    new_of_old = rng.permutation(len(v)).astype(np.int32)
    v2 = np.empty_like(v)
    v2[new_of_old] = v
    return v2, new_of_old[f][rng.permutation(len(f))].astype(np.int32), new_of_old
