"""numpy restatement of the mesh edge table, the topology report and the smoothing (csrc/mesh.hip, cer-mvs_amd/mesh.py mesh_edges /
mesh_topology / smooth_mesh), written from the contract in include/cer_mvs.h with other algorithms than the device's: the
table by np.unique on lo * nv + hi with np.bincount per direction, the neighbour list by np.lexsort, the boundary loops by a union-find,
and the smoothing step as a plain Python loop per vertex in fp64 scalars (never np.sum)."""
import numpy as np

import mesh_reference as M

METHODS = ("taubin", "laplacian")
BOUNDARIES = ("fixed", "free")
TOPOLOGY_KEYS = ("vertices", "faces", "edges", "boundary_edges", "nonmanifold_edges", "inconsistent_edges", "boundary_vertices",
                 "unreferenced_vertices", "degenerate_faces", "boundary_loops", "euler", "closed", "edge_manifold", "oriented")


def as_vertices(vertices):
    return np.ascontiguousarray(np.asarray(vertices, dtype=np.float32).reshape(-1, 3))


def as_faces(faces):
    return np.ascontiguousarray(np.asarray(faces, dtype=np.int32).reshape(-1, 3))


def edge_table(faces, nv):
    """(lo, hi, n_lo_hi, n_hi_lo) int32, ordered by (lo, hi): the undirected edges and the directed edges on them, per direction"""
    f = as_faces(faces).astype(np.int64)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    a, b = a[a != b], b[a != b]                              # a directed edge with equal ends is skipped
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    uniq, inv = np.unique(lo * max(nv, 1) + hi, return_inverse=True)
    inv = inv.reshape(-1)
    forward = np.bincount(inv[a < b], minlength=len(uniq))
    backward = np.bincount(inv[a > b], minlength=len(uniq))
    return tuple(x.astype(np.int32) for x in (uniq // max(nv, 1), uniq % max(nv, 1), forward, backward))


def mesh_edges(faces, nv):
    """(nbr_starts int32 [nv + 1], nbrs, along, against int32 [nn]): every edge from both ends, sorted by (owner, neighbour)"""
    lo, hi, fw, bw = edge_table(faces, nv)
    owner = np.concatenate([lo, hi])
    other = np.concatenate([hi, lo])
    along, against = np.concatenate([fw, bw]), np.concatenate([bw, fw])
    order = np.lexsort((other, owner))
    starts = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=nv))]).astype(np.int32)
    return starts, other[order].astype(np.int32), along[order].astype(np.int32), against[order].astype(np.int32)


def boundary_loops(lo, hi, nv):
    """the components of the graph of the given edges that own an edge: union-find with path halving"""
    parent = list(range(nv))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in zip(lo.tolist(), hi.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return len({find(a) for a in lo.tolist()})


def boundary_vertices(faces, nv):
    """bool [nv]: on an edge with exactly one face"""
    lo, hi, fw, bw = edge_table(faces, nv)
    b = (fw + bw) == 1
    mask = np.zeros(nv, dtype=bool)
    mask[lo[b]] = True
    mask[hi[b]] = True
    return mask


def topology(faces, nv):
    f = as_faces(faces)
    lo, hi, fw, bw = edge_table(f, nv)
    n = fw + bw
    b = n == 1
    referenced = np.zeros(nv, dtype=bool)
    referenced[f.reshape(-1)] = True
    nb, nm = int(b.sum()), int((n > 2).sum())
    ni = int(((n == 2) & ((fw == 2) | (bw == 2))).sum())
    nref = int(referenced.sum())
    return dict(vertices=int(nv), faces=len(f), edges=len(lo), boundary_edges=nb, nonmanifold_edges=nm, inconsistent_edges=ni,
                boundary_vertices=int(boundary_vertices(f, nv).sum()), unreferenced_vertices=int(nv) - nref,
                degenerate_faces=int(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).sum()),
                boundary_loops=boundary_loops(lo[b], hi[b], nv), euler=nref - len(lo) + len(f), closed=nb == 0 and len(f) >= 1,
                edge_manifold=nm == 0, oriented=nm == 0 and ni == 0)


def frozen_flags(vertices, faces, boundary="fixed"):
    """(finite bool [nv], frozen bool [nv], boundary bool [nv], neighbour lists) from the input"""
    v = as_vertices(vertices)
    nv = len(v)
    starts, nbrs, _, _ = mesh_edges(faces, nv)
    finite = np.isfinite(v).all(1)
    on_boundary = boundary_vertices(faces, nv)
    lists = [[int(u) for u in nbrs[starts[i]:starts[i + 1]] if finite[u]] for i in range(nv)]
    frozen = np.array([not finite[i] or not lists[i] or (boundary == "fixed" and bool(on_boundary[i])) for i in range(nv)], dtype=bool)
    return finite, frozen, on_boundary, lists


def step(p, lists, frozen, w):
    """one step on the fp64 state p [nv, 3]: a new array"""
    q = p.copy()
    w = float(w)
    for i in range(len(p)):
        if frozen[i]:
            continue
        for a in range(3):
            s = 0.0
            for u in lists[i]:
                s = s + float(p[u, a])
            m = s / float(len(lists[i]))
            q[i, a] = float(p[i, a]) + w * (m - float(p[i, a]))
    return q


def smooth(vertices, faces, iterations, method="taubin", lam=0.5, mu=-0.53, boundary="fixed", states=False):
    """(vertices' float32 [nv, 3], info) - with ``states`` also the fp64 state after the last step"""
    v = as_vertices(vertices)
    finite, frozen, on_boundary, lists = frozen_flags(v, faces, boundary)
    p = v.astype(np.float64)
    steps = 0
    with np.errstate(all="ignore"):
        for _ in range(iterations):
            p = step(p, lists, frozen, lam)
            steps += 1
            if method == "taubin":
                p = step(p, lists, frozen, mu)
                steps += 1
        out = p.astype(np.float32)
    out[frozen] = v[frozen]                                  # a frozen vertex returns its input bits
    info = dict(moved=int((~frozen).sum()), frozen_boundary=int(on_boundary.sum()) if boundary == "fixed" else 0, steps=steps,
                edges=len(edge_table(faces, len(v))[0]))
    return (out, info, p) if states else (out, info)


# ---------------------------------------------------------------- cases
TRIANGLE = [[0, 1, 2]]
TETRAHEDRON = [[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]]
TETRAHEDRON_VERTICES = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.25, 0.5, 1.5]]


def hand_made():
    """name -> (faces, nv, the figures of the report written out by hand (a subset of its keys))"""
    return {
        "an empty mesh": ([], 0, dict(vertices=0, faces=0, edges=0, boundary_edges=0, nonmanifold_edges=0, inconsistent_edges=0, boundary_vertices=0,
                                      unreferenced_vertices=0, degenerate_faces=0, boundary_loops=0, euler=0, closed=False, edge_manifold=True, oriented=True)),
        "one triangle": (TRIANGLE, 3, dict(edges=3, boundary_edges=3, boundary_vertices=3, boundary_loops=1, euler=1, closed=False, oriented=True)),
        "two triangles, consistent": ([[0, 1, 2], [2, 1, 3]], 4, dict(edges=5, boundary_edges=4, inconsistent_edges=0, boundary_loops=1, euler=1, oriented=True)),
        "two triangles, opposite": ([[0, 1, 2], [1, 2, 3]], 4, dict(edges=5, boundary_edges=4, inconsistent_edges=1, nonmanifold_edges=0, edge_manifold=True,
                                                                     oriented=False, euler=1)),
        "three triangles on one edge": ([[0, 1, 2], [1, 0, 3], [0, 1, 4]], 5, dict(edges=7, nonmanifold_edges=1, boundary_edges=6, inconsistent_edges=0,
                                                                                   edge_manifold=False, oriented=False, euler=1)),
        "a face with a repeated index": ([[0, 1, 2], [2, 2, 1]], 3, dict(edges=3, degenerate_faces=1, boundary_edges=2, nonmanifold_edges=1, faces=2,
                                                                        inconsistent_edges=0, boundary_vertices=3, boundary_loops=1, euler=2)),
        "an unreferenced vertex": (TRIANGLE, 5, dict(vertices=5, unreferenced_vertices=2, euler=1, boundary_vertices=3, boundary_loops=1)),
        "two separate triangles": ([[0, 1, 2], [3, 4, 5]], 6, dict(edges=6, boundary_edges=6, boundary_loops=2, euler=2)),
        "a tetrahedron": (TETRAHEDRON, 4, dict(edges=6, boundary_edges=0, nonmanifold_edges=0, inconsistent_edges=0, boundary_vertices=0, boundary_loops=0,
                                               euler=2, closed=True, edge_manifold=True, oriented=True)),
    }


def field_mesh(name):
    """the small analytic meshes of the tests: (vertices, faces, centre or None)"""
    if name == "sphere12":
        tsdf, weight, grid, centre = M.sphere_field(12, 4.2)
    elif name == "sphere24":
        tsdf, weight, grid, centre = M.sphere_field(24, 9.3)
    elif name == "open12":                                   # the 12^3 sphere with its upper slabs unobserved: one boundary loop
        tsdf, weight, grid, centre = M.sphere_field(12, 4.2)
        weight[:, :, 7:] = 0
    elif name == "random":
        tsdf, weight, grid = M.random_volume()
        centre = None
    else:
        raise KeyError(name)
    v, f = M.extract_mesh(tsdf, weight, grid, min_weight=1)
    return v, f, centre


def radial_noise(vertices, centre, radius, seed=11, sigma=0.15):
    """the vertices pushed along their radius by normal(0, sigma) / radius of it"""
    v = np.asarray(vertices, np.float64)
    d = v - centre
    return (centre + d * (1.0 + np.random.default_rng(seed).normal(0.0, sigma, len(v))[:, None] / radius)).astype(np.float32)


def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float((a * np.cross(b, c)).sum() / 6.0)


def sphere_distance_mean(vertices, centre, radius):
    return float(np.abs(np.linalg.norm(np.asarray(vertices, np.float64) - centre, axis=1) - radius).mean())


def renumbered(vertices, faces, seed):
    """the same mesh with its vertices renumbered by a seeded permutation and its faces shuffled: (vertices', faces', new index of every old
    vertex)"""
    rng = np.random.default_rng(seed)
    v, f = as_vertices(vertices), as_faces(faces)
    new_of_old = rng.permutation(len(v)).astype(np.int32)
    v2 = np.empty_like(v)
    v2[new_of_old] = v
    return v2, new_of_old[f][rng.permutation(len(f))].astype(np.int32), new_of_old
