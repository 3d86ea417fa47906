"""Mesh components and small-piece removal on the MI355X (csrc/mesh.hip, cer-mvs_amd/mesh.py) against the union-find
restatement of tests/mesh_clean_reference.py.  Every comparison is exact: component ids, sizes, indices, and the bits of positions and
attributes.  The restatement itself is held to hand-written results and to the three-sphere figures in tests/test_mesh_clean_cpu.py."""
import numpy as np
import pytest
import torch

import mesh_attr_reference as A
import mesh_clean_reference as C
import mesh_reference as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev_components(dev, faces, nv):
    """mesh_components on the device -> (the four arrays on the host, info)"""
    from cer_mvs_amd import mesh as ME
    faces = C.as_faces(faces)
    info = {}
    out = ME.mesh_components(torch.from_numpy(faces).to(dev), nv, info=info)
    assert [t.dtype for t in out] == [torch.int32, torch.int32, torch.int64, torch.int64] and all(t.is_cuda for t in out)
    assert tuple(out[0].shape) == (nv,) and tuple(out[1].shape) == (len(faces),) and out[2].shape == out[3].shape and out[2].dim() == 1
    assert info["components"] == out[2].shape[0] and set(info) == {"components", "sweeps"}
    return tuple(t.cpu().numpy() for t in out), info


def assert_same_components(got, want, what=""):
    for g, w, name in zip(got, want, ("vertex_component", "face_component", "n_faces", "n_vertices")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name)


def dev_select(dev, fn, vertices, faces, *args, normals=None, colors=None, **kw):
    """select_faces / remove_small_components on the device -> the five results on the host (None stays None)"""
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = fn(t(vertices), t(C.as_faces(faces)), *[t(a) if isinstance(a, np.ndarray) else a for a in args], normals=t(normals), colors=t(colors), **kw)
    v, f, index, n, c = out
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and index.dtype == torch.int32 and v.is_cuda and f.is_cuda and index.is_cuda
    assert v.shape == (index.shape[0], 3) and f.dim() == 2 and f.shape[1] == 3
    assert (n is None) == (normals is None) and (c is None) == (colors is None)
    return tuple(None if a is None else a.cpu().numpy() for a in out)


def assert_same_selection(got, want, what=""):
    for g, w, name in zip(got, want, ("vertices", "faces", "index", "normals", "colors")):
        assert (g is None) == (w is None), (what, name)
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == np.ascontiguousarray(w).tobytes(), (what, name)


@pytest.fixture(scope="module")
def spheres():
    """the three-sphere mesh and the restatement's components, computed once and left unchanged"""
    tsdf, weight, grid = C.three_sphere_field()
    v, f = M.extract_mesh(tsdf, weight, grid)
    assert (len(v), len(f)) == (1464, 2916)
    return v, f, C.mesh_components(f, len(v))


# ---------------------------------------------------------------- components
def test_components_equal_the_restatement_on_hand_made_meshes(dev):
    from cer_mvs_amd import mesh as ME
    for name, (faces, nv, by_hand) in C.hand_made().items():
        got, info = dev_components(dev, faces, nv)
        assert_same_components(got, C.mesh_components(C.as_faces(faces), nv), name)
        assert [g.tolist() for g in got] == [list(w) for w in by_hand], name
        assert info["sweeps"] >= (1 if len(faces) and nv else 0) and info["sweeps"] <= nv + 1, name
    got, info = dev_components(dev, [], 0)                                         # nv = 0
    assert all(g.shape == (0,) for g in got) and info == {"components": 0, "sweeps": 0}
    got, info = dev_components(dev, [], 7)                                         # nf = 0 with nv > 0: seven components of one vertex
    assert got[0].tolist() == list(range(7)) and got[1].shape == (0,) and not got[2].any() and got[3].tolist() == [1] * 7 and info["sweeps"] == 0
    for faces in ([[0, 1, 5]], [[0, -1, 2]]):                                      # out-of-range faces: refused, nothing launched
        with pytest.raises(ValueError, match="indices"):
            ME.mesh_components(torch.tensor(faces, dtype=torch.int32, device=dev), 5)


def test_components_of_the_three_spheres_and_a_renumbering(dev, spheres):
    v, f, want = spheres
    got, info = dev_components(dev, f, len(v))
    assert_same_components(got, want)
    assert got[2].tolist() == [1980, 780, 156] and got[3].tolist() == [992, 392, 80] and info["components"] == 3
    f2, new_of_old, face_order = C.renumbered(f, len(v), seed=11)
    got2, info2 = dev_components(dev, f2, len(v))
    assert_same_components(got2, C.mesh_components(f2, len(v)), "renumbered")
    print(f"three spheres: {info['sweeps']} sweeps in slot order, {info2['sweeps']} after a seeded renumbering")
    back = got2[0][new_of_old]                                                     # the partition, mapped back: identical
    pairs = np.unique(np.stack([got[0], back], 1), axis=0)
    assert len(pairs) == 3 and len(set(pairs[:, 0])) == 3 and len(set(pairs[:, 1])) == 3
    assert np.array_equal(got2[1], back[f[face_order][:, 0]])
    by_new_id = pairs[np.argsort(pairs[:, 1]), 0]                                  # the ids follow the new roots
    new_roots = [int(new_of_old[got[0] == c].min()) for c in by_new_id]
    assert new_roots == sorted(new_roots) and new_roots == C.component_roots(f2, len(v)).tolist()
    assert np.array_equal(got2[2], got[2][by_new_id]) and np.array_equal(got2[3], got[3][by_new_id])


@pytest.mark.parametrize("min_weight, parts", [(1, 6), (2, 15)])
def test_components_of_the_random_volume(dev, min_weight, parts):
    tsdf, weight, grid = M.random_volume()
    v, f = M.extract_mesh(tsdf, weight, grid, min_weight=min_weight)
    got, info = dev_components(dev, f, len(v))
    assert_same_components(got, C.mesh_components(f, len(v)))
    print(f"random volume, min_weight {min_weight}: components of {got[2].tolist()} faces, {info['sweeps']} sweeps")
    assert info["components"] == parts and (got[2] <= 4).sum() >= 2               # many tiny ones
    if min_weight == 1:
        assert got[2].tolist() == [1636, 4, 2, 16, 2, 16]


@pytest.mark.parametrize("seed", [None, 5])
def test_components_of_the_strip(dev, seed):
    """4100 triangles (i, i + 1, i + 2): one component, a chain 4101 hops long; with a seeded renumbering the minimum has to travel the chain
    in both directions - the case that one sweep, or a termination test that races, gets wrong"""
    f, nv = C.strip()
    if seed is not None:
        f = C.renumbered(f, nv, seed)[0]
    got, info = dev_components(dev, f, nv)
    print(f"strip of 4100 triangles, numbering seed {seed}: {info['sweeps']} sweeps")
    assert not got[0].any() and not got[1].any() and got[2].tolist() == [4100] and got[3].tolist() == [4102]
    assert 2 <= info["sweeps"] <= nv + 1
    again, info2 = dev_components(dev, f, nv)                                      # two runs: the same bytes (the sweep count may differ)
    assert all(a.tobytes() == g.tobytes() for a, g in zip(again, got))


def test_components_across_compaction_tiles(dev):
    from cer_mvs_amd import mesh as ME
    tsdf, weight, grid, centre = M.sphere_field((65, 64, 64), 24.3)
    v, f = M.extract_mesh(tsdf, weight, grid)
    assert len(v) == 33266 and len(f) == 66528 and len(v) > 16 * ME.MESH_TILE
    got, info = dev_components(dev, f, len(v))
    print(f"65x64x64 sphere field: {info['sweeps']} sweeps")
    assert_same_components(got, C.mesh_components(f, len(v)))
    assert info["components"] == 1 and not got[0].any() and got[2].tolist() == [66528] and got[3].tolist() == [33266]
    again, _ = dev_components(dev, f, len(v))
    assert all(a.tobytes() == g.tobytes() for a, g in zip(again, got))
    # and the selection across tiles: every third face, and the identity
    keep = (np.arange(len(f)) % 3 == 0)
    assert_same_selection(dev_select(dev, ME.select_faces, v, f, keep), C.select_faces(v, f, keep), "every third face")
    sv, sf, index, _, _ = dev_select(dev, ME.select_faces, v, f, np.ones(len(f), bool))
    assert sv.tobytes() == v.tobytes() and sf.tobytes() == f.tobytes() and np.array_equal(index, np.arange(len(v), dtype=np.int32))


# ---------------------------------------------------------------- selection
def test_select_faces_equals_the_restatement(dev, spheres):
    from cer_mvs_amd import mesh as ME
    v, f, (vc, fc, n_faces, n_vertices) = spheres
    rng = np.random.default_rng(2)
    nrm = rng.normal(size=v.shape).astype(np.float32)
    col = rng.integers(0, 256, size=v.shape).astype(np.uint8)
    nf = len(f)
    all_kept = dev_select(dev, ME.select_faces, v, f, np.ones(nf, bool))           # the identity, byte-equal
    assert all_kept[0].tobytes() == v.tobytes() and all_kept[1].tobytes() == f.tobytes() and np.array_equal(all_kept[2], np.arange(len(v), dtype=np.int32))
    none = dev_select(dev, ME.select_faces, v, f, np.zeros(nf, bool), normals=nrm, colors=col)
    assert none[0].shape == (0, 3) and none[1].shape == (0, 3) and none[2].shape == (0,) and none[3].shape == (0, 3) and none[4].shape == (0, 3)
    masks = {"every second face": np.arange(nf) % 2 == 0, "the middle component dropped": fc != 1, "the first component alone": fc == 0,
             "a random third": rng.uniform(size=nf) < 0.33, "one face": np.arange(nf) == 1700}
    for what, keep in masks.items():
        want = C.select_faces(v, f, keep, nrm, col)
        got = dev_select(dev, ME.select_faces, v, f, keep, normals=nrm, colors=col)
        assert_same_selection(got, want, what)
        assert_same_selection(dev_select(dev, ME.select_faces, v, f, keep.astype(np.uint8) * 7), want[:3] + (None, None), what + ", uint8")
        ov, of, index, on, oc = got                                                # the attributes, checked against index
        assert (np.diff(index) > 0).all() and np.array_equal(bits(ov), bits(v[index])) and np.array_equal(bits(on), bits(nrm[index])) and np.array_equal(oc, col[index])
        assert np.array_equal(index[of], f[keep]) and len(of) == int(keep.sum())
    dropped = dev_select(dev, ME.select_faces, v, f, fc != 1)
    assert (len(dropped[0]), len(dropped[1])) == (992 + 80, 1980 + 156)
    # hand-made: unreferenced vertices leave even when every face stays; repeated indices; an empty mesh
    hv = (np.arange(27, dtype=np.float32).reshape(9, 3) * np.float32(0.37)).astype(np.float32)
    hf = C.as_faces([[1, 2, 4], [5, 6, 7], [7, 4, 1], [8, 8, 2]])
    for keep in ([1, 1, 1, 1], [1, 0, 1, 0], [0, 0, 0, 1], [0, 0, 0, 0]):
        keep = np.array(keep, bool)
        assert_same_selection(dev_select(dev, ME.select_faces, hv, hf, keep), C.select_faces(hv, hf, keep), keep.tolist())
    empty = dev_select(dev, ME.select_faces, hv[:0], hf[:0], np.zeros(0, bool))
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3) and empty[2].shape == (0,)
    no_face = dev_select(dev, ME.select_faces, hv, hf[:0], np.zeros(0, bool))
    assert no_face[0].shape == (0, 3) and no_face[1].shape == (0, 3)
    with pytest.raises(ValueError, match="keep"):
        ME.select_faces(torch.from_numpy(hv).to(dev), torch.from_numpy(hf).to(dev), torch.ones(3, dtype=torch.bool, device=dev))
    with pytest.raises(ValueError, match="indices"):
        ME.select_faces(torch.from_numpy(hv[:8]).to(dev), torch.from_numpy(hf).to(dev), torch.ones(4, dtype=torch.bool, device=dev))


def test_select_faces_at_the_boundaries_of_the_compaction(dev):
    """2050 disjoint triangles (6150 vertices) with exactly the faces kept that sit at the seams of compact.hpp's tile walk: the first and last
    lane of a row (0, 63), the next row's first (64), the last and first position of a wave's segment (511, 512), the last position of a tile
    and the first of the next (2047, 2048), and the last face (2049).  An off-by-one in the rank, the row sum, the wave base or the block
    offset moves or drops one of them; the vertex pass crosses the same seams at three times the positions."""
    from cer_mvs_amd import mesh as ME
    assert ME.MESH_TILE == 2048
    nf = 2050
    rng = np.random.default_rng(7)
    v = rng.normal(size=(3 * nf, 3)).astype(np.float32)
    f = np.arange(3 * nf, dtype=np.int32).reshape(nf, 3)
    kept = [0, 63, 64, 511, 512, 2047, 2048, 2049]
    keep = np.zeros(nf, bool)
    keep[kept] = True
    want = C.select_faces(v, f, keep)
    got = dev_select(dev, ME.select_faces, v, f, keep)
    assert_same_selection(got, want, "the seams")
    assert got[2].tolist() == [3 * q + c for q in kept for c in range(3)] and got[1].tolist() == np.arange(24).reshape(8, 3).tolist()


# ---------------------------------------------------------------- removal
def test_remove_small_components_on_the_three_spheres(dev, spheres):
    from cer_mvs_amd import mesh as ME
    v, f, _ = spheres
    cases = (("min_faces = 157", dict(min_faces=157), (1384, 2760), 2), ("keep_largest = 1", dict(keep_largest=1), (992, 1980), 1),
             ("both", dict(min_faces=157, keep_largest=1), (992, 1980), 1), ("both, the size decides", dict(min_faces=781, keep_largest=2), (992, 1980), 1),
             ("keep_largest = 2", dict(keep_largest=2), (1384, 2760), 2), ("nothing is large enough", dict(min_faces=1981), (0, 0), 0),
             ("min_faces = 1", dict(min_faces=1), (1464, 2916), 3), ("keep_largest = 5", dict(keep_largest=5), (1464, 2916), 3))
    for what, kw, size, parts in cases:
        info = {}
        got = dev_select(dev, ME.remove_small_components, v, f, info=info, **kw)
        want, winfo = C.remove_small_components(v, f, **kw)
        assert_same_selection(got, want, what)
        assert (len(got[0]), len(got[1])) == size, what
        sweeps = info.pop("sweeps")
        assert info == winfo and 1 <= sweeps <= len(v) + 1, what
        assert info["removed_components"] == 3 - parts and info["removed_faces"] == 2916 - size[1] and info["removed_vertices"] == 1464 - size[0]
        if size[1]:                                                                # what is left is still closed, and has `parts` parts
            once, closed, edges, boundary = M.edge_stats(got[1], len(got[0]))
            assert once and closed and boundary == 0 and len(got[0]) - edges + len(got[1]) == 2 * parts, what
            assert len(C.mesh_components(got[1], len(got[0]))[2]) == parts
    identity = dev_select(dev, ME.remove_small_components, v, f, min_faces=1)
    assert identity[0].tobytes() == v.tobytes() and identity[1].tobytes() == f.tobytes()
    # min_faces = 1 is the identity apart from unreferenced vertices
    faces, nv, _ = C.hand_made()["unreferenced vertices first, last and in the middle"]
    hv = np.arange(3 * nv, dtype=np.float32).reshape(nv, 3)
    info = {}
    got = dev_select(dev, ME.remove_small_components, hv, faces, min_faces=1, info=info)
    want, winfo = C.remove_small_components(hv, faces, min_faces=1)
    assert_same_selection(got, want)
    assert got[2].tolist() == [1, 2, 4, 5, 6, 7] and {k: info[k] for k in winfo} == winfo and winfo["removed_vertices"] == 3
    # ties under keep_largest: the smaller id first
    faces, nv, _ = C.hand_made()["size ties"]
    hv = np.arange(3 * nv, dtype=np.float32).reshape(nv, 3)
    for k in (1, 2, 3, 4, 9):
        assert_same_selection(dev_select(dev, ME.remove_small_components, hv, faces, keep_largest=k), C.remove_small_components(hv, faces, keep_largest=k)[0], k)
    assert dev_select(dev, ME.remove_small_components, hv, faces, keep_largest=1)[2].tolist() == [3, 4, 5, 6]


def test_attributes_of_the_cleaned_mesh_are_the_full_mesh_s_gathered(dev, spheres):
    """components are vertex-disjoint and colours are per vertex: computed on the cleaned mesh they equal, bit for bit, those of the full mesh
    gathered by index - and those carried through the removal"""
    from cer_mvs_amd import mesh as ME
    v, f, _ = spheres
    depths, masks, Ks, Es = M.sphere_views()
    colors = A.painted_views(depths, masks, Ks, Es, fill=4.0)
    # the three spheres brought into the ten views' sight: x spans about -0.6 .. 1.2 around the views' target
    pv = ((v.astype(np.float64) - np.array([15.0, 6.0, 6.0])) * 0.06 + M.SPHERE_CENTRE).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)
    dv, df = t(pv), t(f)
    full_n = ME.vertex_normals(dv, df)
    full_c, full_seen = ME.vertex_colors(dv, t(depths), t(masks), t(colors), t(Ks), t(Es), 2.5)
    assert int((full_seen > 0).sum()) > 100 and full_c.any()
    for kw in (dict(min_faces=157), dict(keep_largest=1), dict(min_faces=1)):
        cv, cf, index, cn, cc = ME.remove_small_components(dv, df, normals=full_n, colors=full_c, **kw)
        gather = index.long()
        assert torch.equal(cn.view(torch.int32), full_n[gather].view(torch.int32)) and torch.equal(cc, full_c[gather])
        again_n = ME.vertex_normals(cv, cf)
        again_c, again_seen = ME.vertex_colors(cv, t(depths), t(masks), t(colors), t(Ks), t(Es), 2.5)
        assert torch.equal(again_n.view(torch.int32), cn.view(torch.int32)), kw
        assert torch.equal(again_c, cc) and torch.equal(again_seen, full_seen[gather]), kw
        assert np.array_equal(bits(again_n.cpu().numpy()), bits(A.vertex_normals(cv.cpu().numpy(), cf.cpu().numpy()))), kw


# ---------------------------------------------------------------- chain
@pytest.fixture(scope="module")
def plain_scan(dev, tmp_path_factory):
    """reconstruct_scan(mesh={"resolution": 48}) on the small synthetic scan, once, and the restatement's components of its mesh"""
    import test_reconstruct_gpu as TR
    from cer_mvs_amd.scan import reconstruct_scan
    images, poses, intr, scales = TR._scan(128, 160)
    model = TR._model(dev)
    folder = tmp_path_factory.mktemp("plain")
    args = (model, images, poses, intr, TR.NAMES, TR.PAIRS, scales)
    kw = dict(num_frames=TR.NF, streams=2)
    plain = reconstruct_scan(*args, folder, mesh={"resolution": 48}, **kw)
    comps = C.mesh_components(plain["mesh_faces"], len(plain["mesh_vertices"]))
    print(f"reconstruct_scan plain mesh: {plain['mesh_info']['nv']} vertices, {plain['mesh_info']['nf']} faces, {len(comps[2])} components of "
          f"{sorted(comps[2].tolist(), reverse=True)[:12]} ... faces")
    return args, kw, plain, folder, comps


SAME_KEYS = ("xyz", "rgb", "masks", "depth_est")
REMOVAL_KEYS = {"extracted", "components", "removed_components", "removed_faces", "removed_vertices", "sweeps"}


def test_reconstruct_scan_min_component_1_changes_nothing_but_the_info(dev, plain_scan, tmp_path):
    from cer_mvs_amd.scan import reconstruct_scan
    args, kw, plain, folder, comps = plain_scan
    out = reconstruct_scan(*args, tmp_path, mesh={"resolution": 48, "min_component": 1}, **kw)
    assert set(out) == set(plain)
    for k in SAME_KEYS + ("mesh_vertices", "mesh_faces"):
        assert out[k].dtype == plain[k].dtype and out[k].tobytes() == plain[k].tobytes(), k
    info = dict(out["mesh_info"])
    assert set(info) - set(plain["mesh_info"]) == REMOVAL_KEYS
    assert info["extracted"] == (plain["mesh_info"]["nv"], plain["mesh_info"]["nf"]) and info["components"] == len(comps[2])
    assert (info["removed_components"], info["removed_faces"], info["removed_vertices"]) == (0, 0, 0)
    assert {k: info[k] for k in plain["mesh_info"]} == plain["mesh_info"]
    for name in ("result.ply", "result_mesh.ply"):
        assert (tmp_path / name).read_bytes() == (folder / name).read_bytes(), name


def test_reconstruct_scan_min_component_keeps_the_largest_pieces(dev, plain_scan, tmp_path):
    from cer_mvs_amd import mesh as ME
    from cer_mvs_amd.scan import reconstruct_scan
    args, kw, plain, folder, (vc, fc, n_faces, n_vertices) = plain_scan
    k = int(n_faces.max())                                                         # from the restatement on the plain mesh
    tied = int((n_faces == k).sum())
    out = reconstruct_scan(*args, tmp_path, mesh={"resolution": 48, "min_component": k, "normals": True}, **kw)
    for key in SAME_KEYS:                                                          # cloud, masks and depths: byte-equal to the plain run
        assert out[key].dtype == plain[key].dtype and out[key].tobytes() == plain[key].tobytes(), key
    assert (tmp_path / "result.ply").read_bytes() == (folder / "result.ply").read_bytes()
    pv, pf = plain["mesh_vertices"], plain["mesh_faces"]
    direct = dev_select(dev, ME.remove_small_components, pv, pf, min_faces=k)
    want, winfo = C.remove_small_components(pv, pf, min_faces=k)
    assert_same_selection(direct, want)
    v, f, info = out["mesh_vertices"], out["mesh_faces"], out["mesh_info"]
    assert v.tobytes() == want[0].tobytes() and f.tobytes() == want[1].tobytes() and v.dtype == np.float32 and f.dtype == np.int32
    assert (info["nv"], info["nf"]) == (len(v), len(f)) and info["extracted"] == (len(pv), len(pf))
    assert {key: info[key] for key in winfo} == winfo and info["removed_components"] == len(n_faces) - tied
    left = C.mesh_components(f, len(v))                                            # exactly the components tied for largest survive
    assert left[2].tolist() == [k] * tied and len(f) == k * tied
    print(f"reconstruct_scan min_component = {k}: {info}")
    # the normals are those of the returned mesh, and the file holds what was returned
    assert np.array_equal(bits(out["mesh_normals"]), bits(A.vertex_normals(v, f)))
    rv, rf, rn, rc = ME.read_mesh_ply(tmp_path / "result_mesh.ply", attributes=True)
    assert np.array_equal(bits(rv), bits(v)) and np.array_equal(rf, f) and np.array_equal(bits(rn), bits(out["mesh_normals"])) and rc is None
