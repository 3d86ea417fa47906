"""numpy restatement of the mesh hole filling (csrc/mesh_fill.hip, cer-mvs_amd/mesh.py mesh_holes / fill_holes), written
from the contract in include/cer_mvs.h with other algorithms than the device's: the half-edges from a dict of directed edges -> faces, the
holes by whole-cycle extraction with visited marks and the minimum taken afterwards, and the centres as plain Python fp64 scalar sums
(never np.sum)."""
import numpy as np

import mesh_reference as M
import mesh_smooth_reference as S

INFO_KEYS = ("holes", "added_vertices", "added_faces", "pinched_vertices", "boundary_edges_before")
as_vertices, as_faces = S.as_vertices, S.as_faces


def directed_edges(faces):
    """(a, b) -> the faces with the directed edge a->b (one with equal ends is skipped)"""
    table = {}
    for q, (i0, i1, i2) in enumerate(as_faces(faces).tolist()):
        for a, b in ((i0, i1), (i1, i2), (i2, i0)):
            if a != b:
                table.setdefault((a, b), []).append(q)
    return table


def boundary_half_edges(faces):
    """the directed edges a->b that one face runs along and none against, as a sorted list"""
    table = directed_edges(faces)
    return sorted(e for e, along in table.items() if len(along) == 1 and (e[1], e[0]) not in table)


def next_table(faces, nv):
    """int32 [nv]: the head of the one boundary half-edge that leaves a simple vertex, -1 where none touches it, -2 where it is pinched"""
    leaving, entering = [[] for _ in range(nv)], [0] * nv
    for a, b in boundary_half_edges(faces):
        leaving[a].append(b)
        entering[b] += 1
    out = np.full(nv, -1, dtype=np.int32)
    for v in range(nv):
        if leaving[v] or entering[v]:
            out[v] = leaving[v][0] if len(leaving[v]) == 1 and entering[v] == 1 else -2
    return out


def cycles(nxt):
    """every cycle of ``next`` through simple vertices, each rotated to start at its smallest index, ordered by that index"""
    nv = len(nxt)
    visited = [False] * nv
    found = []
    for start in range(nv):
        if visited[start] or nxt[start] < 0:
            continue
        path, u = [], start
        while u >= 0 and not visited[u]:
            visited[u] = True
            path.append(u)
            u = int(nxt[u])
        if u == start:                                       # back where it began: a whole cycle (a chain ends at a pinched vertex instead)
            k = path.index(min(path))
            found.append(path[k:] + path[:k])
    return sorted(found)


def hole_cycles(faces, nv, max_edges, vertices=None):
    """the holes as lists of members a0 (the head) .. a(n-1), heads ascending"""
    finite = None if vertices is None else np.isfinite(as_vertices(vertices)).all(1)
    return [c for c in cycles(next_table(faces, nv)) if 3 <= len(c) <= max_edges and (finite is None or all(finite[a] for a in c))]


def mesh_holes(faces, nv, max_edges, vertices=None):
    """(head int32 [nh], length int32 [nh])"""
    found = hole_cycles(faces, nv, max_edges, vertices)
    return np.array([c[0] for c in found], dtype=np.int32), np.array([len(c) for c in found], dtype=np.int32)


def centre(p, members):
    """float32 [3]: per axis the fp64 sum in member order, starting at 0.0, divided by the count and rounded once"""
    out = np.empty(3, dtype=np.float32)
    for axis in range(3):
        s = 0.0
        for a in members:
            s = s + float(p[a, axis])
        out[axis] = np.float32(s / float(len(members)))
    return out


def fill(vertices, faces, max_edges, colors=None):
    """((vertices', faces', hole, colors' | None), info)"""
    v, f = as_vertices(vertices), as_faces(faces)
    nv = len(v)
    found = hole_cycles(f, nv, max_edges, v)
    new_v, new_f, new_c, hole = [], [], [], [-1] * len(f)
    for h, members in enumerate(found):
        n = len(members)
        if n == 3:
            new_f.append((members[0], members[2], members[1]))
            hole.append(h)
            continue
        c = nv + len(new_v)
        new_v.append(centre(v, members))
        if colors is not None:
            new_c.append([sum(int(colors[a, ch]) for a in members) // n for ch in range(3)])
        for k in range(n):
            new_f.append((members[(k + 1) % n], members[k], c))
            hole.append(h)
    out_v = np.concatenate([v, np.array(new_v, dtype=np.float32).reshape(-1, 3)])
    out_f = np.concatenate([f, np.array(new_f, dtype=np.int32).reshape(-1, 3)])
    out_c = None if colors is None else np.concatenate([np.asarray(colors, np.uint8).reshape(-1, 3), np.array(new_c, dtype=np.uint8).reshape(-1, 3)])
    nxt = next_table(f, nv)
    info = dict(holes=len(found), added_vertices=len(new_v), added_faces=len(new_f), pinched_vertices=int((nxt == -2).sum()),
                boundary_edges_before=S.topology(f, nv)["boundary_edges"])
    return (out_v, out_f, np.array(hole, dtype=np.int32), out_c), info


# ---------------------------------------------------------------- cases
PAIR = [[0, 1, 2], [2, 1, 3]]
PAIR_VERTICES = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.1], [0.0, 1.0, 0.2], [1.0, 1.0, 0.7]]
PAIR_OPPOSITE = [[0, 1, 2], [1, 2, 3]]
FAN_OF_THREE = [[0, 1, 2], [1, 0, 3], [0, 1, 4]]
BOW_TIE = [[0, 1, 2], [0, 3, 4]]


def punched_sphere(n, r, holes, seed=3):
    """the n^3 sphere field with weight = 0 at ``holes`` nodes near the surface: (vertices, faces) of its mesh, and of the unpunched one"""
    tsdf, weight, grid, _ = M.sphere_field(n, r)
    whole = M.extract_mesh(tsdf, weight, grid, min_weight=1)
    near = np.argwhere(np.abs(tsdf) < 0.3)
    for i, j, k in near[np.random.default_rng(seed).choice(len(near), holes, replace=False)]:
        weight[i, j, k] = 0
    return M.extract_mesh(tsdf, weight, grid, min_weight=1), whole


def random_colors(nv, seed=4):
    return np.random.default_rng(seed).integers(0, 256, size=(nv, 3)).astype(np.uint8)
