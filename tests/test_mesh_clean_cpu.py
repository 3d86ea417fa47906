"""Mesh components and small-piece removal (csrc/mesh.hip, cer-mvs_amd/mesh.py), the parts that need no GPU: the four entry
points of ABI 1190 and their argument checks in the documented order, the Python layer's ValueErrors, and the union-find restatement of
tests/mesh_clean_reference.py - which the GPU tests hold the device to, integer for integer - held to results written out by hand and to
the figures of the three-sphere field."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mesh_clean_reference as C
import mesh_reference as M
from conftest import REPO

BIG = 1 << 31
NAMES = ("cer_mesh_label_sweeps_i32", "cer_mesh_select_partials", "cer_mesh_select_count", "cer_mesh_select_emit_f32")


# ---------------------------------------------------------------- ABI
def test_clean_abi_symbols_are_declared_and_bound():
    from cer_mvs_amd import _lib as L
    from cer_mvs_amd import mesh as ME
    hdr = open(os.path.join(REPO, "include", "cer_mvs.h")).read()
    names = L.exported_symbols()
    for n in NAMES:
        assert n in names and re.search(r"\b(int|long) %s\(" % n, hdr), n
        if n != "cer_mesh_select_partials":
            assert L._SIGNATURES[n][0] is L._I and L._SIGNATURES[n][1][-1] is L._P             # a stream: the last argument
    assert L.ABI_VERSION >= 1190 and "ABI 1190" in hdr and len(names) >= 109
    lib = L.load()
    assert lib.cer_abi_version() == L.ABI_VERSION
    src = open(os.path.join(REPO, "cer-mvs_amd", "csrc", "mesh.hip")).read()
    for kernel in ("mesh_label_sweep_kernel", "mesh_select_count_kernel", "mesh_select_vertex_emit_kernel", "mesh_select_face_emit_kernel"):
        assert kernel in src, kernel                                                          # in mesh.hip: mesh.o's flags
    sweep = src[src.index("void mesh_label_sweep_kernel"):src.index("// ---- face selection")]
    assert "atomic" not in sweep and "while" not in sweep and "__syncthreads" not in sweep   # no atomics, no walk, no barrier
    tile = ME.MESH_TILE

    def blocks(v):
        return (v + tile - 1) // tile
    for (nv, nf), want in (((0, 0), 0), ((5, 0), 0), ((0, 5), 0), ((1, 1), 2), ((tile, tile + 1), 3), ((33266, 66528), blocks(33266) + blocks(66528)),
                           ((-1, 4), -1), ((4, -1), -1), ((-1, BIG), -1), ((BIG, 4), -2), ((4, (BIG + 2) // 3), -2), ((BIG - 1, BIG // 3), blocks(BIG - 1) + blocks(BIG // 3))):
        assert lib.cer_mesh_select_partials(nv, nf) == want, (nv, nf)


def test_clean_entry_points_refuse_bad_arguments_in_the_documented_order():
    """every check runs before any launch (the pointers are fake: a launch would fault).  The order: (1) a negative size CER_EINVAL (-1); (2)
    nv or 3 nf >= 2^31 CER_ESHAPE (-2); (3) nothing to do CER_OK; (4) null pointers CER_EINVAL - each case breaks one rule and every later
    one, and gets the earlier rule's answer."""
    from cer_mvs_amd import _lib as L
    lib = L.load()
    fake, null = ctypes.c_void_p(4096), None

    def sweeps(fac=fake, nf=4, starts=fake, order=fake, nv=5, labels=fake, flags=fake, n=3):
        return lib.cer_mesh_label_sweeps_i32(fac, nf, starts, order, nv, labels, flags, n, null)
    sn = dict(fac=null, starts=null, order=null, labels=null, flags=null)
    for kw in (dict(nv=-1), dict(nf=-1), dict(n=-1), dict(nv=-1, nf=BIG), dict(n=-2, nv=BIG)):                                      # 1
        assert sweeps(**kw) == -1 and sweeps(**kw, **sn) == -1, kw
    assert sweeps(nv=BIG) == -2 and sweeps(nv=BIG, **sn) == -2 and sweeps(nv=BIG, n=0) == -2                                         # 2
    assert sweeps(nf=(BIG + 2) // 3) == -2 and sweeps(nf=(BIG + 2) // 3, nv=0) == -2 and sweeps(nf=1 << 62, **sn) == -2
    assert sweeps(nv=0) == 0 and sweeps(nv=0, **sn) == 0 and sweeps(n=0) == 0 and sweeps(n=0, **sn) == 0                             # 3
    assert sweeps(nv=0, nf=BIG // 3) == 0 and sweeps(nv=BIG - 1, n=0) == 0
    for name in sn:                                                                                                               # 4
        assert sweeps(**{name: null}) == -1, name
    assert sweeps(nf=0, starts=null) == -1 and sweeps(nf=0, labels=null) == -1 and sweeps(nf=0, flags=null) == -1 and sweeps(nf=0, **sn) == -1

    def count(fac=fake, nf=4, starts=fake, order=fake, nv=5, keep=fake, used=fake, part=fake, off=fake, tot=fake):
        return lib.cer_mesh_select_count(fac, nf, starts, order, nv, keep, used, part, off, tot, null)
    cn = dict(fac=null, starts=null, order=null, keep=null, used=null, part=null, off=null, tot=null)
    for kw in (dict(nv=-1), dict(nf=-1), dict(nv=-1, nf=BIG)):                                                                     # 1
        assert count(**kw) == -1 and count(**kw, **cn) == -1, kw
    assert count(nv=BIG) == -2 and count(nv=BIG, **cn) == -2 and count(nf=(BIG + 2) // 3) == -2 and count(nf=(BIG + 2) // 3, nv=0) == -2   # 2
    for kw in (dict(nv=0), dict(nf=0), dict(nv=0, nf=0), dict(nv=BIG - 1, nf=0)):                                                  # 3
        assert count(**kw) == 0 and count(**kw, **cn) == 0, kw
    for name in cn:                                                                                                               # 4
        assert count(**{name: null}) == -1, name

    def emit(ver=fake, nv=5, fac=fake, nf=4, keep=fake, used=fake, off=fake, nvo=5, nfo=4, vmap=fake, out=fake, index=fake, outf=fake):
        return lib.cer_mesh_select_emit_f32(ver, nv, fac, nf, keep, used, off, nvo, nfo, vmap, out, index, outf, null)
    en = dict(ver=null, fac=null, keep=null, used=null, off=null, vmap=null, out=null, index=null, outf=null)
    for kw in (dict(nv=-1), dict(nf=-1), dict(nvo=-1), dict(nfo=-1), dict(nvo=-1, nv=BIG)):                                        # 1
        assert emit(**kw) == -1 and emit(**kw, **en) == -1, kw
    assert emit(nv=BIG) == -2 and emit(nv=BIG, **en) == -2 and emit(nf=(BIG + 2) // 3, nvo=0, nfo=0) == -2                           # 2
    for kw in (dict(nv=0), dict(nf=0), dict(nvo=0, nfo=0)):                                                                       # 3
        assert emit(**kw) == 0 and emit(**kw, **en) == 0, kw
    for name in en:                                                                                                               # 4
        assert emit(**{name: null}) == -1, name
    assert emit(nfo=0, out=null) == -1 and emit(nfo=0, index=null) == -1 and emit(nvo=0, outf=null) == -1
    assert emit(nfo=0, outf=null, ver=null) == -1 and emit(nvo=0, out=null, index=null, vmap=null) == -1


# ---------------------------------------------------------------- the Python layer
def test_clean_python_layer_refuses_bad_arguments_without_a_device():
    from cer_mvs_amd import mesh as ME
    from cer_mvs_amd.scan import reconstruct_scan
    ver = torch.zeros(5, 3)
    fac = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32)
    keep = torch.tensor([True, False])
    nrm, col = torch.zeros(5, 3), torch.zeros(5, 3, dtype=torch.uint8)
    for bad in (fac.long(), fac[:, :2], fac[0], fac.numpy()):
        with pytest.raises(ValueError, match="faces"):
            ME.mesh_components(bad, 5)
        with pytest.raises(ValueError, match="faces"):
            ME.select_faces(ver, bad, keep)
        with pytest.raises(ValueError, match="faces"):
            ME.remove_small_components(ver, bad, min_faces=1)
    for bad in (torch.tensor([[0, 1, 5]], dtype=torch.int32), torch.tensor([[0, -1, 2]], dtype=torch.int32)):                     # out-of-range faces
        with pytest.raises(ValueError, match="indices"):
            ME.mesh_components(bad, 5)
        with pytest.raises(ValueError, match="indices"):
            ME.select_faces(ver, bad, keep[:1])
        with pytest.raises(ValueError, match="indices"):
            ME.remove_small_components(ver, bad, keep_largest=1)
    with pytest.raises(ValueError, match="indices"):
        ME.mesh_components(fac, 3)
    with pytest.raises(ValueError, match="nv"):
        ME.mesh_components(fac, -1)
    for bad in (ver.double(), ver[:, :2], ver[0], ver.numpy()):
        with pytest.raises(ValueError, match="vertices"):
            ME.select_faces(bad, fac, keep)
        with pytest.raises(ValueError, match="vertices"):
            ME.remove_small_components(bad, fac, min_faces=1)
    for bad in (keep[:1], torch.ones(3, dtype=torch.bool), keep.int(), keep.float(), keep[None], [True, False], None):         # a wrong-size keep
        with pytest.raises(ValueError, match="keep"):
            ME.select_faces(ver, fac, bad)
    for bad in (nrm[:4], nrm.double(), nrm[:, :2], nrm.numpy()):
        with pytest.raises(ValueError, match="normals"):
            ME.select_faces(ver, fac, keep, normals=bad)
        with pytest.raises(ValueError, match="normals"):
            ME.remove_small_components(ver, fac, min_faces=1, normals=bad)
    for bad in (col[:4], col.float(), col[:, :2]):
        with pytest.raises(ValueError, match="colors"):
            ME.select_faces(ver, fac, keep, colors=bad)
    with pytest.raises(ValueError, match="min_faces or keep_largest"):                                                          # a missing criterion
        ME.remove_small_components(ver, fac)
    for bad in (0, -1, True, False, 2.0, 1.5, "3", [1]):
        with pytest.raises(ValueError, match="min_faces"):
            ME.remove_small_components(ver, fac, min_faces=bad)
        with pytest.raises(ValueError, match="keep_largest"):
            ME.remove_small_components(ver, fac, keep_largest=bad)
        with pytest.raises(ValueError, match="keep_largest"):
            ME.remove_small_components(ver, fac, min_faces=2, keep_largest=bad)
    for call in (lambda: ME.mesh_components(fac, 5), lambda: ME.select_faces(ver, fac, keep, normals=nrm, colors=col),
                 lambda: ME.select_faces(ver, fac, keep.to(torch.uint8)), lambda: ME.remove_small_components(ver, fac, min_faces=1),
                 lambda: ME.remove_small_components(ver, fac, min_faces=3, keep_largest=2, normals=nrm, colors=col)):
        with pytest.raises(RuntimeError, match="CUDA"):      # good arguments: the host tensors are what is refused
            call()
    # the options of reconstruct_scan(mesh=...): refused before a model or a session is built
    for key in ("min_component", "keep_largest"):
        for bad in (0, -3, True, False, 2.0, 0.5, "2", None, [2]):
            with pytest.raises(ValueError, match="mesh: " + key):
                ME.mesh_options({key: bad})
            with pytest.raises(ValueError, match="mesh: " + key):
                reconstruct_scan(None, [0], [0], [0], ["a"], [[0]], [1.0], None, write=False, mesh={"resolution": 48, key: bad})
    for bad in ({"min_faces": 3}, {"min_components": 3}, {"keep_biggest": 1}):
        with pytest.raises(ValueError, match="unknown"):
            ME.mesh_options(bad)
    for good in ({"min_component": 1}, {"keep_largest": 1}, {"resolution": 48, "min_component": 157, "keep_largest": 2, "colors": True, "normals": True}):
        assert ME.mesh_options(good) == good
    assert {"min_component", "keep_largest"} <= set(ME.MESH_OPTION_KEYS)


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", sorted(C.hand_made()))
def test_restated_components_on_hand_made_meshes(name):
    faces, nv, want = C.hand_made()[name]
    got = C.mesh_components(C.as_faces(faces), nv)
    assert [g.dtype for g in got] == [np.int32, np.int32, np.int64, np.int64]
    for g, w, what in zip(got, want, ("vertex_component", "face_component", "n_faces", "n_vertices")):
        assert g.tolist() == list(w), (name, what)
    assert int(got[2].sum()) == len(faces) and int(got[3].sum()) == nv
    # another face order and another index order inside the faces: the same partition
    f = C.as_faces(faces)
    again = C.mesh_components(f[::-1][:, [2, 0, 1]], nv)
    assert again[0].tolist() == list(want[0]) and again[2].tolist() == list(want[2]) and again[3].tolist() == list(want[3])


def test_restated_selection_on_hand_made_meshes():
    v = (np.arange(27, dtype=np.float32).reshape(9, 3) * np.float32(0.37)).astype(np.float32)
    f = C.as_faces([[1, 2, 4], [5, 6, 7], [7, 4, 1], [8, 8, 2]])
    nrm, col = -v, (np.arange(27).reshape(9, 3) * 7 % 256).astype(np.uint8)
    ov, of, index, on, oc = C.select_faces(v, f, [True, False, True, False], nrm, col)
    assert index.tolist() == [1, 2, 4, 7] and index.dtype == np.int32 and of.dtype == np.int32 and ov.dtype == np.float32
    assert of.tolist() == [[0, 1, 2], [3, 2, 0]]
    assert np.array_equal(ov, v[index]) and np.array_equal(on, nrm[index]) and np.array_equal(oc, col[index])
    ov, of, index, on, oc = C.select_faces(v, f, np.ones(4, bool))                 # all kept: the unreferenced vertices 0 and 3 leave
    assert index.tolist() == [1, 2, 4, 5, 6, 7, 8] and of.tolist() == [[0, 1, 2], [3, 4, 5], [5, 2, 0], [6, 6, 1]] and on is None and oc is None
    ov, of, index, _, _ = C.select_faces(v, f, np.zeros(4, np.uint8))
    assert ov.shape == (0, 3) and of.shape == (0, 3) and index.shape == (0,)
    ov, of, index, _, _ = C.select_faces(v[:0], f[:0], np.zeros(0, bool))
    assert ov.shape == (0, 3) and of.shape == (0, 3) and index.shape == (0,)


def test_restated_removal_and_size_ties():
    faces, nv, _ = C.hand_made()["size ties"]
    f = C.as_faces(faces)
    v = np.arange(3 * nv, dtype=np.float32).reshape(nv, 3)
    n_faces = C.mesh_components(f, nv)[2]
    assert n_faces.tolist() == [1, 2, 2, 1]
    for k, want in ((1, [1]), (2, [1, 2]), (3, [0, 1, 2]), (4, [0, 1, 2, 3]), (9, [0, 1, 2, 3])):       # ties: the smaller id first
        assert np.flatnonzero(C.kept_components(n_faces, keep_largest=k)).tolist() == want, k
    assert np.flatnonzero(C.kept_components(n_faces, min_faces=2)).tolist() == [1, 2]
    assert np.flatnonzero(C.kept_components(n_faces, min_faces=2, keep_largest=1)).tolist() == [1]
    assert np.flatnonzero(C.kept_components(n_faces, min_faces=3, keep_largest=3)).tolist() == []
    (ov, of, index, _, _), info = C.remove_small_components(v, f, keep_largest=1)
    assert index.tolist() == [3, 4, 5, 6] and of.tolist() == [[0, 1, 2], [0, 2, 3]]
    assert info == dict(components=4, removed_components=3, removed_faces=4, removed_vertices=10)
    (ov, of, index, _, _), info = C.remove_small_components(v, f, min_faces=1)
    assert np.array_equal(ov, v) and np.array_equal(of, f) and info["removed_components"] == 0
    # a faceless component counts as removed under min_faces and is never a vertex of the result
    faces, nv, _ = C.hand_made()["unreferenced vertices first, last and in the middle"]
    (ov, of, index, _, _), info = C.remove_small_components(np.zeros((nv, 3), np.float32), C.as_faces(faces), min_faces=1)
    assert index.tolist() == [1, 2, 4, 5, 6, 7] and info == dict(components=4, removed_components=3, removed_faces=0, removed_vertices=3)
    (ov, of, index, _, _), info = C.remove_small_components(np.zeros((nv, 3), np.float32), C.as_faces(faces), keep_largest=3)
    assert index.tolist() == [1, 2, 4, 5, 6, 7] and info["removed_components"] == 1 and info["removed_vertices"] == 3


def test_restated_components_of_the_three_sphere_field():
    tsdf, weight, grid = C.three_sphere_field()
    assert grid[2] == (30, 13, 12)
    v, f = M.extract_mesh(tsdf, weight, grid)
    assert (len(v), len(f)) == (1464, 2916)
    vc, fc, n_faces, n_vertices = C.mesh_components(f, len(v))
    assert C.component_roots(f, len(v)).tolist() == [0, 124, 466]
    assert n_faces.tolist() == [1980, 780, 156] and n_vertices.tolist() == [992, 392, 80]
    for c in range(3):                                                             # each part alone: a closed surface of genus 0
        pv, pf, index, _, _ = C.select_faces(v, f, fc == c)
        assert (len(pv), len(pf)) == (int(n_vertices[c]), int(n_faces[c])) and (vc[index] == c).all()
        (once, closed, edges, boundary), chi = C.submesh_closed(pv, pf)
        assert once and closed and boundary == 0 and chi == 2 and edges == 3 * len(pf) // 2, c
    (pv, pf, _, _, _), info = C.remove_small_components(v, f, min_faces=157)
    # 992 + 392 = 1384 vertices: two closed genus-0 parts with 2760 faces have 4 + 4140 - 2760 of them, whatever the algorithm
    assert (len(pv), len(pf)) == (1384, 2760) and info ==dict(components=3, removed_components=1, removed_faces=156, removed_vertices=80)
    (pv, pf, _, _, _), info = C.remove_small_components(v, f, keep_largest=1)
    assert (len(pv), len(pf)) == (992, 1980) and info["removed_components"] == 2
    # renumbered and shuffled: the same partition, numbered by the new roots
    f2, new_of_old, face_order = C.renumbered(f, len(v), seed=11)
    vc2, fc2, nf2, nv2 = C.mesh_components(f2, len(v))
    back = vc2[new_of_old]                                                         # the new numbering's component of every old vertex
    pairs = np.unique(np.stack([vc, back], 1), axis=0)
    assert len(pairs) == 3                                                         # a bijection between the two numberings
    assert sorted(nf2.tolist()) == [156, 780, 1980] and np.array_equal(nf2[pairs[:, 1]], n_faces[pairs[:, 0]]) and np.array_equal(nv2[pairs[:, 1]], n_vertices[pairs[:, 0]])
    assert np.array_equal(fc2, back[f[face_order][:, 0]])
    roots2 = C.component_roots(f2, len(v))
    assert [int(new_of_old[vc == c].min()) for c in pairs[np.argsort(pairs[:, 1]), 0]] == roots2.tolist()


@pytest.mark.parametrize("min_weight, parts, sizes", [(1, 6, [1636, 4, 2, 16, 2, 16]), (2, 15, None)])
def test_restated_components_of_the_random_volume(min_weight, parts, sizes):
    tsdf, weight, grid = M.random_volume()
    v, f = M.extract_mesh(tsdf, weight, grid, min_weight=min_weight)
    vc, fc, n_faces, n_vertices = C.mesh_components(f, len(v))
    print(f"random volume, min_weight {min_weight}: {len(v)} vertices, {len(f)} faces, components of {n_faces.tolist()} faces")
    assert len(n_faces) == parts and int(n_faces.sum()) == len(f) and (n_faces > 0).all()              # every vertex of an extraction is referenced
    if sizes is not None:
        assert len(f) == 1676 and n_faces.tolist() == sizes
    # the partition by its definition: no face joins two components, and every component is connected through its faces' shared vertices
    assert (vc[f[:, 0]] == vc[f[:, 1]]).all() and (vc[f[:, 0]] == vc[f[:, 2]]).all()
    label = np.arange(len(v))
    for _ in range(len(v)):                                                        # np.minimum.at to a fixed point: a third algorithm
        before = label.copy()
        m = label[f].min(1)
        for c in range(3):
            np.minimum.at(label, f[:, c], m)
        if np.array_equal(before, label):
            break
    assert np.array_equal(np.searchsorted(np.unique(label), label), vc)


def test_restated_components_of_the_strip():
    f, nv = C.strip()
    assert (len(f), nv) == (4100, 4102)
    for faces in (f, C.renumbered(f, nv, seed=5)[0]):
        vc, fc, n_faces, n_vertices = C.mesh_components(faces, nv)
        assert not vc.any() and not fc.any() and n_faces.tolist() == [4100] and n_vertices.tolist() == [4102]
