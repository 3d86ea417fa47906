"""numpy restatement of the mesh cleaning (csrc/mesh.hip, cer-mvs_amd/mesh.py), written from the contract in include/cer_mvs.h
with ANOTHER algorithm than the device's label sweeps: a plain union-find over the faces (path halving, the smaller root wins), a boolean
scatter for the surviving vertices and a cumulative sum for their new indices.  Plus the cases the tests share: hand-made meshes, the
three-sphere field, the triangle strip and seeded renumberings."""
import numpy as np

import mesh_reference as M


def vertex_roots(faces, nv):
    """int64 [nv]: the smallest vertex index of every vertex's component"""
    parent = list(range(nv))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    def union(a, b):
        ra, rb = find(a), find(b)
        if ra < rb:
            parent[rb] = ra
        elif rb < ra:
            parent[ra] = rb
    for a, b, c in np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist():
        union(a, b)
        union(a, c)
    return np.array([find(v) for v in range(nv)], dtype=np.int64).reshape(nv)


def mesh_components(faces, nv):
    """(vertex_component int32 [nv], face_component int32 [nf], n_faces int64 [nc], n_vertices int64 [nc]); ``roots`` are np.unique of
    vertex_roots"""
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    root = vertex_roots(faces, nv)
    roots = np.unique(root)                                   # ascending: the numbering
    vc = np.searchsorted(roots, root).astype(np.int32)
    fc = vc[faces[:, 0]].astype(np.int32)
    nc = len(roots)
    return vc, fc, np.bincount(fc, minlength=nc).astype(np.int64), np.bincount(vc, minlength=nc).astype(np.int64)


def component_roots(faces, nv):
    return np.unique(vertex_roots(faces, nv))


def select_faces(vertices, faces, keep, normals=None, colors=None):
    """(vertices', faces', index int32 [nv'], normals' | None, colors' | None)"""
    vertices = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    keep = np.asarray(keep).astype(bool)
    kept = faces[keep]
    used = np.zeros(len(vertices), dtype=bool)
    used[kept.reshape(-1)] = True
    new = np.cumsum(used) - 1
    index = np.flatnonzero(used).astype(np.int32)
    return (vertices[index], new[kept].astype(np.int32).reshape(-1, 3), index, None if normals is None else np.asarray(normals)[index],
            None if colors is None else np.asarray(colors)[index])


def kept_components(n_faces, min_faces=None, keep_largest=None):
    """bool [nc]: n_faces >= min_faces where given, and among the first keep_largest by (n_faces descending, id ascending) where given"""
    assert min_faces is not None or keep_largest is not None
    nc = len(n_faces)
    kept = np.ones(nc, dtype=bool)
    if min_faces is not None:
        kept &= n_faces >= min_faces
    if keep_largest is not None:
        ranked = sorted(range(nc), key=lambda c: (-int(n_faces[c]), c))
        first = np.zeros(nc, dtype=bool)
        first[ranked[:keep_largest]] = True
        kept &= first
    return kept


def remove_small_components(vertices, faces, min_faces=None, keep_largest=None, normals=None, colors=None):
    """(select_faces' five results, info)"""
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    nv = len(vertices)
    _, fc, n_faces, _ = mesh_components(faces, nv)
    kept = kept_components(n_faces, min_faces, keep_largest)
    out = select_faces(vertices, faces, kept[fc], normals, colors)
    info = dict(components=len(n_faces), removed_components=int((~kept).sum()), removed_faces=len(faces) - len(out[1]), removed_vertices=nv - len(out[0]))
    return out, info


# ---------------------------------------------------------------- cases
def hand_made():
    """name -> (faces, nv, the expected (vertex_component, face_component, n_faces, n_vertices) written out by hand)"""
    return {
        "an empty mesh": ([], 0, ([], [], [], [])),
        "no face, three vertices": ([], 3, ([0, 1, 2], [], [0, 0, 0], [1, 1, 1])),
        "one triangle": ([[0, 1, 2]], 3, ([0, 0, 0], [0], [1], [3])),
        "two disjoint triangles": ([[0, 1, 2], [5, 4, 3]], 6, ([0, 0, 0, 1, 1, 1], [0, 1], [1, 1], [3, 3])),
        "two triangles sharing one vertex": ([[0, 1, 2], [2, 3, 4]], 5, ([0, 0, 0, 0, 0], [0, 0], [2], [5])),
        "unreferenced vertices first, last and in the middle": ([[1, 2, 4], [5, 6, 7], [7, 4, 1]], 9,
                                                                ([0, 1, 1, 2, 1, 1, 1, 1, 3], [1, 1, 1], [0, 3, 0, 0], [1, 6, 1, 1])),
        "faces with repeated indices": ([[0, 0, 1], [2, 2, 2], [3, 4, 3], [4, 4, 5], [6, 1, 6]], 8,
                                        ([0, 0, 1, 2, 2, 2, 0, 3], [0, 1, 2, 2, 0], [2, 1, 2, 0], [3, 1, 3, 1])),
        "interleaved numbering": ([[6, 1, 3], [0, 2, 4], [5, 3, 7], [4, 8, 2]], 9, ([0, 1, 0, 1, 0, 1, 1, 1, 0], [1, 0, 1, 0], [2, 2], [4, 5])),
        "size ties": ([[0, 1, 2], [3, 4, 5], [3, 5, 6], [7, 8, 9], [7, 9, 10], [11, 12, 13]], 14,
                      ([0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3], [0, 1, 1, 2, 2, 3], [1, 2, 2, 1], [3, 4, 4, 3])),
    }


def as_faces(faces):
    return np.asarray(faces, dtype=np.int32).reshape(-1, 3)


THREE_SPHERES = (((5.8, 6.0, 5.6), 4.2), ((16.3, 6.2, 5.4), 2.7), ((24.9, 5.7, 6.1), 1.3))


def three_sphere_field(dims=(30, 13, 12)):
    """the pointwise minimum of three sphere distances on a unit grid, weight 1: (tsdf, weight, grid)"""
    f = None
    for centre, r in THREE_SPHERES:
        t, weight, grid, _ = M.sphere_field(dims, r, centre=centre)
        f = t if f is None else np.minimum(f, t)
    return f, weight, grid


def strip(n=4100):
    """n triangles (i, i + 1, i + 2) over n + 2 vertices: one component, a chain n + 1 hops long"""
    i = np.arange(n, dtype=np.int32)
    return np.stack([i, i + 1, i + 2], 1), n + 2


def renumbered(faces, nv, seed):
    """the same mesh with its vertices renumbered by a seeded permutation and its faces shuffled: (faces', new index of every old vertex,
    old position of every new face)"""
    rng = np.random.default_rng(seed)
    new_of_old = rng.permutation(nv).astype(np.int32)
    face_order = rng.permutation(len(faces))
    return new_of_old[as_faces(faces)][face_order].astype(np.int32), new_of_old, face_order


def submesh_closed(vertices, faces):
    """(edge_stats of the faces, Euler characteristic) of a mesh whose vertices are all referenced"""
    return M.edge_stats(faces, len(vertices)), M.euler_characteristic(vertices, faces)
