"""Mesh simplification by vertex clustering (csrc/mesh.hip, cer-mvs_amd/mesh.py simplify_vertex_clustering), the parts that
need no GPU: the four entry points of ABI 1200 and their argument checks in the documented order, the Python layer's ValueErrors and the
forms of the "simplify" option, and the numpy restatement of tests/mesh_simplify_reference.py - which the GPU tests hold the device to, bit
for bit - held to results written out by hand, to np.linalg.solve, to the guarantees of the contract and to the figures of the analytic
sphere meshes (profiles/mesh_simplify_parity.json)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mesh_reference as M
import mesh_simplify_reference as S
from conftest import REPO

BIG = 1 << 31
NAMES = ("cer_mesh_cluster_map_i32", "cer_mesh_cluster_reps_f32", "cer_mesh_cluster_faces_i32", "cer_mesh_face_heads_u8")
INFO_KEYS = {"clusters", "degenerate_faces", "duplicate_faces", "dropped_clusters", "quadric"}


# ---------------------------------------------------------------- ABI
def test_simplify_abi_symbols_are_declared_and_bound():
    from cer_mvs_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "cer_mvs.h")).read()
    names = L.exported_symbols()
    for n in NAMES:
        assert n in names and re.search(r"\bint %s\(" % n, hdr), n
        assert L._SIGNATURES[n][0] is L._I and L._SIGNATURES[n][1][-1] is L._P                 # a stream: the last argument
    assert L.ABI_VERSION >= 1200 and "Mesh simplification (ABI 1200" in hdr and len(names) >= 113
    for doc in ("README.md", "DESIGN.md"):
        assert f"{len(names)} entry points" in open(os.path.join(REPO, doc)).read(), doc
    lib = L.load()
    assert lib.cer_abi_version() == L.ABI_VERSION
    src = open(os.path.join(REPO, "cer-mvs_amd", "csrc", "mesh.hip")).read()
    for kernel in ("mesh_cluster_map_kernel", "mesh_cluster_reps_kernel", "mesh_cluster_faces_kernel", "mesh_face_heads_kernel"):
        assert "void " + kernel in src, kernel                                                # in mesh.hip: mesh.o's flags
    section = src[src.index("// ---- simplification by vertex clustering"):]
    assert not re.search(r"atomic\w*\s*\(|__shared__|__syncthreads|\bfmaf?\s*\(", section)      # no atomics, no LDS, no barrier, no fused multiply-add


def test_simplify_entry_points_refuse_bad_arguments_in_the_documented_order():
    """every check runs before any launch (the pointers are fake: a launch would fault).  The order: (1) a negative size CER_EINVAL (-1); (2)
    nv, 3 nf or ncells >= 2^31, or ncells > nv CER_ESHAPE (-2); (3) the origin non-finite, cell or regularisation not positive and finite
    CER_EINVAL; (4) nothing to do CER_OK; (5) null pointers CER_EINVAL - each case breaks one rule and every later one, and gets the earlier
    rule's answer."""
    from cer_mvs_amd import _lib as L
    lib = L.load()
    fake, null = ctypes.c_void_p(4096), None
    third = (BIG + 2) // 3
    inf, nan = float("inf"), float("nan")

    def vec(*v):
        return (ctypes.c_double * 3)(*v)

    def cmap(order=fake, start=fake, nv=5, nc=3, cluster=fake):
        return lib.cer_mesh_cluster_map_i32(order, start, nv, nc, cluster, null)
    mn = dict(order=null, start=null, cluster=null)
    for kw in (dict(nv=-1), dict(nc=-1), dict(nv=-1, nc=BIG), dict(nc=-1, nv=BIG)):                                                  # 1
        assert cmap(**kw) == -1 and cmap(**kw, **mn) == -1, kw
    for kw in (dict(nv=BIG), dict(nv=BIG + 5, nc=BIG), dict(nc=6), dict(nv=0), dict(nv=0, nc=1)):                                     # 2 (ncells > nv)
        assert cmap(**kw) == -2 and cmap(**kw, **mn) == -2, kw
    assert cmap(nv=0, nc=0) == 0 and cmap(nv=0, nc=0, **mn) == 0                                                                      # 4
    for name in mn:                                                                                                                   # 5
        assert cmap(**{name: null}) == -1 and cmap(nc=0, **{name: null}) == -1, name

    def reps(ver=fake, nv=5, fac=fake, nf=4, starts=fake, corder=fake, order=fake, start=fake, keys=fake, nc=3, origin=vec(0.0, 0.0, 0.0), cell=1.0,
             quadric=1, reg=1e-3, col=fake, out=fake, outc=fake, took=fake):
        return lib.cer_mesh_cluster_reps_f32(ver, nv, fac, nf, starts, corder, order, start, keys, nc, origin, cell, quadric, reg, col, out, outc,
                                             took, null)
    rn = dict(ver=null, fac=null, starts=null, corder=null, order=null, start=null, keys=null, col=null, out=null, outc=null, took=null)
    for kw in (dict(nv=-1), dict(nf=-1), dict(nc=-1), dict(nv=-1, nf=BIG), dict(nc=-1, cell=0.0)):                                    # 1
        assert reps(**kw) == -1 and reps(**kw, **rn) == -1, kw
    for kw in (dict(nv=BIG), dict(nf=third), dict(nc=6), dict(nv=BIG + 1, nc=BIG), dict(nf=third, cell=nan), dict(nc=6, reg=0.0), dict(nv=0)):     # 2
        assert reps(**kw) == -2 and reps(**kw, **rn) == -2, kw
    for kw in (dict(origin=vec(nan, 0.0, 0.0)), dict(origin=vec(0.0, inf, 0.0)), dict(origin=vec(0.0, 0.0, -inf)), dict(origin=None), dict(cell=0.0),
               dict(cell=-1.0), dict(cell=inf), dict(cell=nan), dict(reg=0.0), dict(reg=-1e-3), dict(reg=inf), dict(reg=nan), dict(reg=nan, quadric=0)):   # 3
        assert reps(**kw) == -1 and reps(**kw, nc=0) == -1 and reps(**kw, nc=0, **{k: v for k, v in rn.items() if k not in kw}) == -1, kw
    assert reps(nc=0) == 0 and reps(nc=0, **rn) == 0 and reps(nc=0, nv=0, nf=0, **rn) == 0 and reps(nc=0, quadric=0, **rn) == 0            # 4
    for name in ("ver", "order", "start", "keys", "out", "took", "starts", "fac", "corder"):                                           # 5
        assert reps(**{name: null}) == -1, name
    assert reps(col=null) == -1 and reps(outc=null) == -1                   # the colours: null together or not at all
    assert reps(nf=0, starts=null, fac=null, corder=null) == -1             # the quadric form walks starts even without a face
    assert reps(quadric=0, ver=null) == -1 and reps(quadric=0, took=null, fac=null, starts=null, corder=null) == -1

    def cfaces(fac=fake, nf=4, cluster=fake, nv=5, triples=fake, valid=fake):
        return lib.cer_mesh_cluster_faces_i32(fac, nf, cluster, nv, triples, valid, null)
    fn = dict(fac=null, cluster=null, triples=null, valid=null)
    for kw in (dict(nf=-1), dict(nv=-1), dict(nf=-1, nv=BIG)):                                                                        # 1
        assert cfaces(**kw) == -1 and cfaces(**kw, **fn) == -1, kw
    for kw in (dict(nv=BIG), dict(nf=third), dict(nf=1 << 62), dict(nf=0, nv=BIG)):                                                   # 2
        assert cfaces(**kw) == -2 and cfaces(**kw, **fn) == -2, kw
    assert cfaces(nf=0) == 0 and cfaces(nf=0, **fn) == 0 and cfaces(nf=0, nv=0, **fn) == 0                                            # 4
    for name in fn:                                                                                                                   # 5
        assert cfaces(**{name: null}) == -1, name

    def heads(triples=fake, valid=fake, perm=fake, nf=4, keep=fake):
        return lib.cer_mesh_face_heads_u8(triples, valid, perm, nf, keep, null)
    hn = dict(triples=null, valid=null, perm=null, keep=null)
    assert heads(nf=-1) == -1 and heads(nf=-1, **hn) == -1                                                                            # 1
    assert heads(nf=third) == -2 and heads(nf=third, **hn) == -2 and heads(nf=1 << 62, **hn) == -2                                    # 2
    assert heads(nf=0) == 0 and heads(nf=0, **hn) == 0                                                                                # 4
    for name in hn:                                                                                                                   # 5
        assert heads(**{name: null}) == -1, name


# ---------------------------------------------------------------- the Python layer
def test_simplify_python_layer_refuses_bad_arguments_without_a_device():
    from cer_mvs_amd import mesh as ME
    from cer_mvs_amd.scan import reconstruct_scan
    ver = torch.zeros(5, 3)
    fac = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32)
    col = torch.zeros(5, 3, dtype=torch.uint8)
    fn = ME.simplify_vertex_clustering
    for bad in (ver.double(), ver[:, :2], ver[0], ver.numpy(), None):
        with pytest.raises(ValueError, match="vertices"):
            fn(bad, fac, 1.0)
    for bad in (fac.long(), fac[:, :2], fac[0], fac.numpy(), None):
        with pytest.raises(ValueError, match="faces"):
            fn(ver, bad, 1.0)
    for bad in (torch.tensor([[0, 1, 5]], dtype=torch.int32), torch.tensor([[0, -1, 2]], dtype=torch.int32)):                     # out-of-range faces
        with pytest.raises(ValueError, match="indices"):
            fn(ver, bad, 1.0)
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), True, "1", None, [1.0]):
        with pytest.raises(ValueError, match="cell"):
            fn(ver, fac, bad)
        with pytest.raises(ValueError, match="regularisation"):
            fn(ver, fac, 1.0, regularisation=bad)
        with pytest.raises(ValueError, match="regularisation"):
            fn(ver, fac, 1.0, representative="mean", regularisation=bad)
    for bad in ("median", "Quadric", "", None, 1, True):
        with pytest.raises(ValueError, match="representative"):
            fn(ver, fac, 1.0, representative=bad)
    for bad in (col[:4], col.float(), col[:, :2], col.numpy(), col.reshape(-1)):
        with pytest.raises(ValueError, match="colors"):
            fn(ver, fac, 1.0, colors=bad)
    for call in (lambda: fn(ver, fac, 1.0), lambda: fn(ver, fac, 2, representative="mean", regularisation=1, colors=col), lambda: fn(ver[:0], fac[:0], 0.5),
                 lambda: fn(ver, fac, np.float32(0.5), info={})):
        with pytest.raises(RuntimeError, match="CUDA"):      # good arguments: the host tensors are what is refused
            call()
    # the option of reconstruct_scan(mesh=...): refused before a model or a session is built
    bad_options = (0, -2, 0.0, float("inf"), float("nan"), True, False, "2", None, [2], {}, {"voxels": 2, "cell": 0.1}, {"representative": "mean"},
                   {"voxels": 0}, {"voxels": True}, {"cell": -1.0}, {"cell": float("nan")}, {"voxels": 2, "representative": "median"},
                   {"voxels": 2, "regularisation": 0}, {"cell": 0.1, "regularisation": float("inf")}, {"voxels": 2, "cells": 3}, {"voxels": "2"})
    for bad in bad_options:
        with pytest.raises(ValueError, match="mesh: simplify"):
            ME.mesh_options({"simplify": bad})
        with pytest.raises(ValueError, match="mesh: simplify"):
            reconstruct_scan(None, [0], [0], [0], ["a"], [[0]], [1.0], None, write=False, mesh={"resolution": 48, "simplify": bad})
    for bad in ({"simplification": 2}, {"simplify_voxels": 2}, {"decimate": 2}):
        with pytest.raises(ValueError, match="unknown"):
            ME.mesh_options(bad)
    for good in ({"simplify": 2}, {"simplify": 1.5}, {"simplify": {"voxels": 2}}, {"simplify": {"cell": 0.05}},
                 {"simplify": {"voxels": 3, "representative": "mean"}}, {"simplify": {"cell": 0.05, "representative": "quadric", "regularisation": 1e-2}},
                 {"resolution": 48, "min_component": 157, "keep_largest": 2, "simplify": 2, "colors": True, "normals": True}):
        assert ME.mesh_options(good) == good
    assert "simplify" in ME.MESH_OPTION_KEYS and ME.mesh_options(True) == {} and ME.mesh_options({"resolution": 48}) == {"resolution": 48}
    assert ME._simplify_option(2) == (2.0, None, "quadric", 1e-3) and ME._simplify_option({"cell": 0.5, "representative": "mean"}) == (None, 0.5, "mean", 1e-3)
    doc = fn.__doc__
    assert "vertex_normals" in doc and "manifold" in doc and "Euler" in doc


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", sorted(S.hand_made()))
def test_restated_simplification_on_hand_made_meshes(name):
    vertices, faces, cell, want, winfo = S.hand_made()[name]
    (v, f, cluster, colors), info = S.simplify(vertices, faces, cell, "mean")
    assert v.dtype == np.float32 and f.dtype == np.int32 and cluster.dtype == np.int32 and colors is None
    assert v.shape == (len(want[0]), 3) and f.shape == (len(want[1]), 3) and cluster.shape == (len(vertices),)
    assert v.tobytes() == S.as_vertices(want[0]).tobytes(), name
    assert f.tolist() == S.as_faces(want[1]).tolist() and cluster.tolist() == list(want[2]) and info == winfo, name
    assert set(info) == INFO_KEYS and info["degenerate_faces"] + info["duplicate_faces"] + len(f) == len(faces)
    (qv, qf, qcluster, _), qinfo = S.simplify(vertices, faces, cell, "quadric")                # the faces do not depend on the representative
    assert qf.tolist() == f.tolist() and qcluster.tolist() == cluster.tolist() and {k: qinfo[k] for k in qinfo if k != "quadric"} == {k: info[k] for k in info if k != "quadric"}
    assert np.isfinite(qv).all() and (np.abs(qv.astype(np.float64) - v) <= cell).all()        # inside the cell of the mean
    # colours: the integer mean of the members
    if len(vertices):
        col = (np.arange(3 * len(vertices)).reshape(-1, 3) * 37 % 256).astype(np.uint8)
        (_, _, _, oc), _ = S.simplify(vertices, faces, cell, "mean", colors=col)
        for out_index in range(len(v)):
            members = np.flatnonzero(cluster == out_index)
            assert oc[out_index].tolist() == [int(col[members, a].astype(np.int64).sum()) // len(members) for a in range(3)], name
        assert oc.dtype == np.uint8 and oc.shape == v.shape


def test_restated_lower_face_index_survives_and_orientation_is_kept():
    vertices, faces, cell, _, _ = S.hand_made()["a fan that collapses to a duplicate pair"]
    (v, f, cluster, _), info = S.simplify(vertices, faces, cell, "mean")
    assert f.tolist() == [[0, 1, 2]] and info["duplicate_faces"] == 1
    # the duplicate first: it is now the lower index, and the same triple survives once
    (v2, f2, _, _), info2 = S.simplify(vertices, faces[::-1], cell, "mean")
    assert f2.tolist() == [[0, 1, 2]] and info2 == info and v2.tobytes() == v.tobytes()
    # surviving faces keep their input order, whatever their triples' order
    quad = S.QUAD
    (_, f3, _, _), _ = S.simplify(quad, [[2, 1, 3], [0, 1, 2]], 1.0, "mean")
    assert f3.tolist() == [[1, 3, 2], [0, 1, 2]]
    # the orientation of every surviving face is its input face's
    sv, sf, _ = S.sphere_mesh()
    (ov, of, cluster, _), _ = S.simplify(sv, sf, 1.5, "mean")
    assert S.up_to_rotation(of) <= S.up_to_rotation(cluster[sf][(cluster[sf] >= 0).all(1)])


def test_restated_cramer_equals_linalg_solve():
    """the regularised systems of the 12^3 sphere at four cells: cond <= 3 / regularisation + 1 = 3001, so the fp64 error is about 1e-12 of |x| <=
    cell; the bar of 1e-9 cell leaves three orders of margin"""
    sv, sf, _ = S.sphere_mesh()
    worst = 0.0
    for cell in (1.0, 1.5, 2.0, 3.0):
        _, _, took, parts = S.representatives(sv, sf, cell, "quadric")
        assert took.sum() > 0.8 * len(took) and (parts["lam"] > 0).all() and (parts["det"] > 0).all()
        # (largest eigenvalue + lam) / (smallest + lam) <= (trace + lam) / lam = 3 / regularisation + 1
        assert np.linalg.cond(parts["mat"]).max() <= (3.0 / 1e-3 + 1.0) * (1 + 1e-9)
        x = np.linalg.solve(parts["mat"], parts["rhs"][:, :, None])[:, :, 0]
        err = float(np.abs(x - parts["x"])[took].max())
        worst = max(worst, err / cell)
        assert err <= 1e-9 * cell, (cell, err)
    print(f"Cramer against np.linalg.solve: at most {worst:.3e} cell")


SPHERE_12 = {1.0: (259, 523, 1), 1.5: (119, 236, 2), 2.0: (68, 133, 1), 3.0: (26, 50, 2)}       # cell -> vertices, faces, duplicates


@pytest.mark.parametrize("cell", sorted(SPHERE_12))
def test_restated_simplification_of_the_sphere(cell):
    sv, sf, centre = S.sphere_mesh()
    assert (len(sv), len(sf)) == (970, 1936) and S.closed(sf, len(sv))
    occupied = len(np.unique(np.floor((sv.astype(np.float64) - sv.astype(np.float64).min(0)) / cell), axis=0))
    sizes = {}
    for representative in S.REPRESENTATIVES:
        (v, f, cluster, _), info = S.simplify(sv, sf, cell, representative)
        print(f"12^3 sphere, cell {cell}, {representative}: {len(v)} vertices, {len(f)} faces, {info}")
        assert S.guarantees(v, f) == (True, True, True)
        assert S.closed(f, len(v))                                                             # closedness is kept
        assert len(v) == occupied == info["clusters"] and info["dropped_clusters"] == 0 and (cluster >= 0).all()
        assert info["degenerate_faces"] + info["duplicate_faces"] + len(f) == len(sf)
        assert (len(v), len(f), info["duplicate_faces"]) == SPHERE_12[cell]
        assert np.array_equal(np.unique(cluster), np.arange(len(v)))                          # ascending cluster order, every one referenced
        sizes[representative] = (f.tolist(), cluster.tolist())
        if representative == "quadric":
            assert 0.85 * len(v) <= info["quadric"] <= len(v)
    assert sizes["mean"] == sizes["quadric"]


@pytest.mark.parametrize("cell, recorded", [(1.0, 0.369), (1.5, 0.403)])
def test_restated_quadric_representatives_lie_closer_to_the_sphere(cell, recorded):
    """24^3 nodes, r = 9.3: the quadric representatives' mean distance to the sphere is below 0.6 of the mean representatives' (the prototype
    of the contract gave 0.37 and 0.40; the cap leaves margin for the written-out associations), and their maximum does not exceed the
    mean's.  This restatement gives 0.369 at cell 1.0 (mean 4.96e-3 against 1.344e-2, maxima 3.165e-2 against 3.233e-2, 1266 of 1339
    clusters take the minimiser) and 0.403 at cell 1.5 (9.33e-3 against 2.316e-2, maxima 3.667e-2 against 4.352e-2, 588 of 597)."""
    sv, sf, centre = S.sphere_mesh(24, 9.3)
    assert (len(sv), len(sf)) == (4848, 9692)
    d = {}
    for representative in S.REPRESENTATIVES:
        (v, f, _, _), info = S.simplify(sv, sf, cell, representative)
        d[representative] = S.sphere_distances(v, centre, 9.3)
        assert S.guarantees(v, f) == (True, True, True) and S.closed(f, len(v))
    ratio = float(d["quadric"].mean() / d["mean"].mean())
    print(f"24^3 sphere, cell {cell}: mean distance {d['quadric'].mean():.4e} (quadric) / {d['mean'].mean():.4e} (mean) = {ratio:.3f}; "
          f"maxima {d['quadric'].max():.4e} / {d['mean'].max():.4e}")
    assert ratio < 0.6 and d["quadric"].max() <= d["mean"].max()
    assert abs(ratio - recorded) < 5e-3                                                        # what profiles/mesh_simplify_parity.json records


def test_restated_simplification_of_the_random_volume_and_a_renumbering():
    tsdf, weight, grid = M.random_volume()
    rv, rf = M.extract_mesh(tsdf, weight, grid, min_weight=1)
    assert len(rf) == 1676
    for cell in (0.37, 0.8):
        (v, f, cluster, _), info = S.simplify(rv, rf, cell, "quadric")
        print(f"random volume, cell {cell}: {len(rv)} -> {len(v)} vertices, {len(rf)} -> {len(f)} faces, {info}")
        assert S.guarantees(v, f) == (True, True, True) and info["degenerate_faces"] + info["duplicate_faces"] + len(f) == len(rf)
        assert len(v) == info["clusters"] - info["dropped_clusters"] and np.isfinite(v).all()
    # renumbered vertices and shuffled faces: the clusters are the same sets, and the same faces survive up to their order
    sv, sf, _ = S.sphere_mesh()
    v2, f2, new_of_old = S.renumbered(sv, sf, seed=3)
    (a_v, a_f, a_cluster, _), a_info = S.simplify(sv, sf, 1.5, "quadric")
    (b_v, b_f, b_cluster, _), b_info = S.simplify(v2, f2, 1.5, "quadric")
    assert np.array_equal(b_cluster[new_of_old], a_cluster) and S.up_to_rotation(a_f) == S.up_to_rotation(b_f)
    assert {k: a_info[k] for k in ("clusters", "degenerate_faces", "duplicate_faces", "dropped_clusters")} == {k: b_info[k] for k in ("clusters", "degenerate_faces", "duplicate_faces", "dropped_clusters")}
    assert np.abs(a_v.astype(np.float64) - b_v).max() < 1e-5                                   # sums in another order: close, not bit-equal
