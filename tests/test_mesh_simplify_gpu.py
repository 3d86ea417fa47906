"""Mesh simplification by vertex clustering on the MI355X (csrc/mesh.hip, cer-mvs_amd/mesh.py simplify_vertex_clustering)
against the numpy restatement of tests/mesh_simplify_reference.py.  Every comparison is exact: positions as bits, faces, the cluster map and
colours as integers, and the info figures.  The restatement itself is held to hand-written results, to np.linalg.solve and to the contract's
guarantees in tests/test_mesh_simplify_cpu.py."""
import numpy as np
import pytest
import torch

import mesh_attr_reference as A
import mesh_reference as M
import mesh_simplify_reference as S

pytestmark = pytest.mark.gpu

INFO_KEYS = {"clusters", "degenerate_faces", "duplicate_faces", "dropped_clusters", "quadric"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def painted(nv, seed=4):
    return np.random.default_rng(seed).integers(0, 256, size=(nv, 3)).astype(np.uint8)


def dev_simplify(dev, vertices, faces, cell, representative, colors=None, **kw):
    """simplify_vertex_clustering on the device -> ((vertices', faces', cluster, colors' | None) on the host, info)"""
    from cer_mvs_amd import mesh as ME
    v, f = S.as_vertices(vertices), S.as_faces(faces)
    info = {}
    out = ME.simplify_vertex_clustering(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), cell, representative=representative,
                                        colors=None if colors is None else torch.from_numpy(colors).to(dev), info=info, **kw)
    ov, of, cluster, oc = out
    assert ov.dtype == torch.float32 and of.dtype == torch.int32 and cluster.dtype == torch.int32 and ov.is_cuda and of.is_cuda and cluster.is_cuda
    assert ov.dim() == 2 and ov.shape[1] == 3 and of.dim() == 2 and of.shape[1] == 3 and tuple(cluster.shape) == (len(v),)
    assert (oc is None) == (colors is None) and (oc is None or (oc.dtype == torch.uint8 and oc.shape == ov.shape and oc.is_cuda))
    assert set(info) == INFO_KEYS
    return tuple(None if a is None else a.cpu().numpy() for a in out), info


def assert_same(got, want, what=""):
    (g, ginfo), (w, winfo) = got, want
    for a, b, name in zip(g, w, ("vertices", "faces", "cluster", "colors")):
        assert (a is None) == (b is None), (what, name)
        if a is not None:
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == np.ascontiguousarray(b).tobytes(), (what, name)
    assert ginfo == winfo, what


def check_both(dev, vertices, faces, cell, what, colors=None):
    """both representatives against the restatement -> {representative: ((arrays), info)} of the device"""
    out = {}
    for representative in S.REPRESENTATIVES:
        out[representative] = dev_simplify(dev, vertices, faces, cell, representative, colors=colors)
        assert_same(out[representative], S.simplify(vertices, faces, cell, representative, colors=colors), (what, representative))
    return out


@pytest.fixture(scope="module")
def sphere():
    """the 12^3 sphere mesh, computed once and left unchanged"""
    v, f, centre = S.sphere_mesh()
    assert (len(v), len(f)) == (970, 1936)
    return v, f, centre


# ---------------------------------------------------------------- against the restatement
def test_simplify_equals_the_restatement_on_hand_made_meshes(dev):
    for name, (vertices, faces, cell, want, winfo) in S.hand_made().items():
        col = painted(len(vertices)) if len(vertices) else None
        out = check_both(dev, vertices, faces, cell, name, colors=col)
        (v, f, cluster, _), info = out["mean"]
        assert v.tobytes() == S.as_vertices(want[0]).tobytes() and f.tolist() == S.as_faces(want[1]).tolist(), name     # and what was written out by hand
        assert cluster.tolist() == list(want[2]) and info == winfo, name
    (v, f, cluster, _), info = dev_simplify(dev, [], [], 1.0, "quadric")                         # nv = 0
    assert v.shape == (0, 3) and f.shape == (0, 3) and cluster.shape == (0,) and not any(info.values())
    out = check_both(dev, S.QUAD, [], 1.0, "nf = 0 with nv > 0", colors=painted(4))              # no face: every cluster is dropped
    (v, f, cluster, oc), info = out["quadric"]
    assert v.shape == (0, 3) and f.shape == (0, 3) and oc.shape == (0, 3) and cluster.tolist() == [-1] * 4
    assert info == dict(clusters=4, degenerate_faces=0, duplicate_faces=0, dropped_clusters=4, quadric=0)


@pytest.mark.parametrize("cell, size", [(1.0, (259, 523, 1)), (1.5, (119, 236, 2)), (2.0, (68, 133, 1)), (3.0, (26, 50, 2))])
def test_simplify_of_the_sphere(dev, sphere, cell, size):
    from cer_mvs_amd import mesh as ME
    sv, sf, centre = sphere
    out = check_both(dev, sv, sf, cell, f"sphere at {cell}", colors=painted(len(sv)))
    for representative, ((v, f, cluster, oc), info) in out.items():
        assert (len(v), len(f), info["duplicate_faces"]) == size and info["dropped_clusters"] == 0
        assert S.guarantees(v, f) == (True, True, True) and S.closed(f, len(v))
        assert info["degenerate_faces"] + info["duplicate_faces"] + len(f) == len(sf)
    d_mean = S.sphere_distances(out["mean"][0][0], centre, 4.2)
    d_quad = S.sphere_distances(out["quadric"][0][0], centre, 4.2)
    print(f"12^3 sphere, cell {cell}: {size[0]} vertices, {size[1]} faces; distance to the sphere mean / max: quadric {d_quad.mean():.4f} / {d_quad.max():.4f}, "
          f"mean {d_mean.mean():.4f} / {d_mean.max():.4f}; {out['quadric'][1]['quadric']} clusters took the minimiser")
    assert d_quad.mean() < d_mean.mean()
    # two runs: the same bytes
    again = dev_simplify(dev, sv, sf, cell, "quadric", colors=painted(len(sv)))
    assert_same(again, out["quadric"], "second run")
    # vertex_normals on the result: finite everywhere (every vertex is referenced), unit length or - where the faces around a vertex cancel - zero
    v, f = out["quadric"][0][:2]
    normals = ME.vertex_normals(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)).cpu().numpy()
    assert np.isfinite(normals).all() and np.array_equal(bits(normals), bits(A.vertex_normals(v, f)))
    length = np.linalg.norm(normals.astype(np.float64), axis=1)
    assert ((np.abs(length - 1.0) < 1e-6) | (length == 0.0)).all() and (length > 0).sum() > 0.9 * len(v)


@pytest.mark.parametrize("cell", [0.2, 0.37, 0.8])
def test_simplify_of_the_random_volume(dev, cell):
    """non-manifold, many tiny pieces, clusters that lose every face"""
    tsdf, weight, grid = M.random_volume()
    rv, rf = M.extract_mesh(tsdf, weight, grid, min_weight=1)
    assert len(rf) == 1676
    out = check_both(dev, rv, rf, cell, f"random volume at {cell}", colors=painted(len(rv), seed=8))
    (v, f, cluster, _), info = out["quadric"]
    print(f"random volume, cell {cell}: {len(rv)} -> {len(v)} vertices, {len(rf)} -> {len(f)} faces, {info}")
    assert S.guarantees(v, f) == (True, True, True) and len(v) == info["clusters"] - info["dropped_clusters"]
    if cell >= 0.37:
        assert info["dropped_clusters"] > 0 and (cluster == -1).any()


def test_simplify_of_a_renumbered_sphere(dev, sphere):
    """vertices renumbered by a seeded permutation, faces shuffled: the contract is the restatement of the PERMUTED input (the member order
    changes, so sums do); the clusters are the same sets, and where a cluster has one member its mean is the same bits"""
    sv, sf, _ = sphere
    v2, f2, new_of_old = S.renumbered(sv, sf, seed=3)
    for cell in (1.0, 2.0):
        plain = check_both(dev, sv, sf, cell, "plain")
        perm = check_both(dev, v2, f2, cell, "renumbered")
        for representative in S.REPRESENTATIVES:
            (av, af, ac, _), ainfo = plain[representative]
            (bv, bf, bc, _), binfo = perm[representative]
            assert np.array_equal(bc[new_of_old], ac) and S.up_to_rotation(af) == S.up_to_rotation(bf), (cell, representative)
            assert {k: ainfo[k] for k in ainfo if k != "quadric"} == {k: binfo[k] for k in binfo if k != "quadric"}
            assert np.abs(av.astype(np.float64) - bv).max() < 1e-5
        (av, _, ac, _), _ = plain["mean"]
        (bv, _, _, _), _ = perm["mean"]
        alone = np.flatnonzero(np.bincount(ac, minlength=len(av)) == 1)
        if cell == 1.0:
            assert len(alone) > 0
        assert np.array_equal(bits(av[alone]), bits(bv[alone]))


def test_simplify_with_a_cell_larger_than_the_mesh_and_one_smaller_than_every_gap(dev, sphere):
    sv, sf, _ = sphere
    for representative in S.REPRESENTATIVES:
        (v, f, cluster, _), info = dev_simplify(dev, sv, sf, 64.0, representative)
        assert v.shape == (0, 3) and f.shape == (0, 3) and (cluster == -1).all()
        assert info == dict(clusters=1, degenerate_faces=len(sf), duplicate_faces=0, dropped_clusters=1, quadric=info["quadric"]) and info["quadric"] <= 1
    cell = 1e-3
    assert S.simplify(sv, sf, cell, "mean")[1]["clusters"] == len(sv)                        # every vertex alone
    out = check_both(dev, sv, sf, cell, "a tiny cell")
    (v, f, cluster, _), info = out["mean"]
    assert info == dict(clusters=len(sv), degenerate_faces=0, duplicate_faces=0, dropped_clusters=0, quadric=0)
    assert np.array_equal(bits(v[cluster]), bits(sv))                                        # every position: its input vertex, bit for bit
    relabelled = cluster[sf]
    first = relabelled.argmin(1)
    rotated = np.stack([relabelled[np.arange(len(sf)), (first + k) % 3] for k in range(3)], 1)
    assert np.array_equal(f, rotated)                                                        # the faces: the input's, relabelled and rotated


def test_simplify_with_planted_non_finite_vertices(dev, sphere):
    sv, sf, _ = sphere
    v = sv.copy()
    v[[0, 17, 400], [0, 1, 2]] = np.nan
    v[[5, 969], [2, 0]] = [np.inf, -np.inf]
    for cell in (1.0, 2.0):
        out = check_both(dev, v, sf, cell, f"non-finite vertices at {cell}", colors=painted(len(v)))
        for (ov, of, cluster, _), info in out.values():
            assert (cluster[[0, 17, 400, 5, 969]] == -1).all() and np.isfinite(ov).all() and S.guarantees(ov, of) == (True, True, True)
            assert info["degenerate_faces"] >= S.simplify(sv, sf, cell, "mean")[1]["degenerate_faces"] + (2 if cell == 1.0 else 0)
    none = check_both(dev, np.full((4, 3), np.nan, np.float32), [[0, 1, 2], [2, 1, 3]], 1.0, "no finite vertex")
    assert none["quadric"][1] == dict(clusters=0, degenerate_faces=2, duplicate_faces=0, dropped_clusters=0, quadric=0)


def test_simplify_across_compaction_tiles(dev):
    """65 x 64 x 64 nodes: 33 266 vertices - more than one 2048-tile in the cell table and in both selection passes"""
    from cer_mvs_amd import mesh as ME
    tsdf, weight, grid, centre = M.sphere_field((65, 64, 64), 24.3)
    v, f = M.extract_mesh(tsdf, weight, grid)
    assert len(v) == 33266 and len(f) == 66528
    out = check_both(dev, v, f, 2.0, "65x64x64 sphere at 2 voxels", colors=painted(len(v)))
    (ov, of, cluster, _), info = out["quadric"]
    print(f"65x64x64 sphere, cell 2: {len(ov)} vertices, {len(of)} faces, {info}")
    assert (len(ov), len(of)) == (2448, 4982) and info["clusters"] > ME.MESH_TILE and len(of) > 2 * ME.MESH_TILE and len(v) > 16 * ME.MESH_TILE
    assert S.guarantees(ov, of) == (True, True, True) and S.closed(of, len(ov))
    assert_same(dev_simplify(dev, v, f, 2.0, "quadric", colors=painted(len(v))), out["quadric"], "second run")
    d_mean = S.sphere_distances(out["mean"][0][0], centre, 24.3)
    d_quad = S.sphere_distances(ov, centre, 24.3)
    print(f"distance to the sphere mean / max: quadric {d_quad.mean():.5f} / {d_quad.max():.5f}, mean {d_mean.mean():.5f} / {d_mean.max():.5f}")
    assert d_quad.mean() < d_mean.mean() and d_quad.max() <= d_mean.max()


def test_simplify_refuses_bad_arguments_on_the_device(dev, sphere):
    from cer_mvs_amd import mesh as ME
    sv, sf, _ = sphere
    v, f = torch.from_numpy(sv).to(dev), torch.from_numpy(sf).to(dev)
    with pytest.raises(ValueError, match="indices"):
        ME.simplify_vertex_clustering(v[:900], f, 1.0)
    with pytest.raises(ValueError, match="one device"):
        ME.simplify_vertex_clustering(v, f.cpu(), 1.0)
    with pytest.raises(ValueError, match="2\\^20"):
        ME.simplify_vertex_clustering(v, f, 1e-6)
    with pytest.raises(ValueError, match="representative"):
        ME.simplify_vertex_clustering(v, f, 1.0, representative="median")


def test_mesh_simplify_tool_carries_colours_and_recomputes_normals(dev, sphere, tmp_path, monkeypatch, capsys):
    """tools/mesh_simplify.py, run in this process: a file with normals and colours in, the simplified mesh with both out"""
    import importlib.util
    import json
    import os
    from conftest import REPO
    from cer_mvs_amd import mesh as ME
    sv, sf, _ = sphere
    col = painted(len(sv))
    spec = importlib.util.spec_from_file_location("mesh_simplify_tool", os.path.join(REPO, "tools", "mesh_simplify.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    src, dst = tmp_path / "in.ply", tmp_path / "out.ply"
    (wv, wf, _, wc), winfo = S.simplify(sv, sf, 1.5, "mean", colors=col)
    for normals_in, flag, normals_out in ((True, [], True), (False, [], False), (False, ["--normals"], True)):
        ME.write_mesh_ply(src, sv, sf, normals=A.vertex_normals(sv, sf) if normals_in else None, colors=col)
        monkeypatch.setattr("sys.argv", ["mesh_simplify.py", str(src), str(dst), "--cell", "1.5", "--representative", "mean"] + flag)
        tool.main()
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert line["vertices"] == len(wv) and line["faces"] == len(wf) and line["read"] == [len(sv), len(sf)] and {k: line[k] for k in winfo} == winfo
        rv, rf, rn, rc = ME.read_mesh_ply(dst, attributes=True)
        assert np.array_equal(bits(rv), bits(wv)) and np.array_equal(rf, wf) and np.array_equal(rc, wc)
        assert (rn is not None) == normals_out and (rn is None or np.array_equal(bits(rn), bits(A.vertex_normals(wv, wf))))


# ---------------------------------------------------------------- chain
SAME_KEYS = ("xyz", "rgb", "masks", "depth_est")
PLAIN_INFO = {"grid", "trunc", "nv", "nf", "observed"}


def test_reconstruct_scan_simplify(dev, tmp_path):
    import test_reconstruct_gpu as TR
    from cer_mvs_amd import mesh as ME
    from cer_mvs_amd.scan import reconstruct_scan
    images, poses, intr, scales = TR._scan(128, 160)
    model = TR._model(dev)
    args = (model, images, poses, intr, TR.NAMES, TR.PAIRS, scales)
    kw = dict(num_frames=TR.NF, streams=2)
    plain_dir, simple_dir = tmp_path / "plain", tmp_path / "simple"
    plain_dir.mkdir()
    simple_dir.mkdir()
    plain = reconstruct_scan(*args, plain_dir, mesh={"resolution": 48}, **kw)
    assert set(plain["mesh_info"]) == PLAIN_INFO and "mesh_normals" not in plain                 # without "simplify": no new key
    out = reconstruct_scan(*args, simple_dir, mesh={"resolution": 48, "simplify": 2, "normals": True}, **kw)
    for key in SAME_KEYS:                                                                        # cloud, masks and depths: byte-equal to the plain run
        assert out[key].dtype == plain[key].dtype and out[key].tobytes() == plain[key].tobytes(), key
    assert (simple_dir / "result.ply").read_bytes() == (plain_dir / "result.ply").read_bytes()
    pv, pf = plain["mesh_vertices"], plain["mesh_faces"]
    voxel = plain["mesh_info"]["grid"].voxel
    direct = dev_simplify(dev, pv, pf, 2 * voxel, "quadric")
    want = S.simplify(pv, pf, 2 * voxel, "quadric")
    assert_same(direct, want, "the plain mesh, simplified")
    v, f, info = out["mesh_vertices"], out["mesh_faces"], out["mesh_info"]
    assert v.dtype == np.float32 and f.dtype == np.int32 and v.tobytes() == want[0][0].tobytes() and f.tobytes() == want[0][1].tobytes()
    assert (info["nv"], info["nf"]) == (len(v), len(f)) and info["simplified_from"] == (len(pv), len(pf))
    assert set(info) - PLAIN_INFO == INFO_KEYS | {"simplified_from"} and {k: info[k] for k in INFO_KEYS} == want[1]
    assert {k: info[k] for k in ("grid", "trunc", "observed")} == {k: plain["mesh_info"][k] for k in ("grid", "trunc", "observed")}
    assert 0 < len(v) < len(pv) / 2 and 0 < len(f) < len(pf) / 2
    print(f"reconstruct_scan simplify = 2: {len(pv)} -> {len(v)} vertices, {len(pf)} -> {len(f)} faces, {info}")
    # the normals are those of the returned mesh, and the file holds what was returned
    assert np.array_equal(bits(out["mesh_normals"]), bits(A.vertex_normals(v, f)))
    rv, rf, rn, rc = ME.read_mesh_ply(simple_dir / "result_mesh.ply", attributes=True)
    assert np.array_equal(bits(rv), bits(v)) and np.array_equal(rf, f) and np.array_equal(bits(rn), bits(out["mesh_normals"])) and rc is None
    # the dictionary form in world units with the mean
    again = reconstruct_scan(*args, None, write=False, mesh={"resolution": 48, "simplify": {"cell": 2 * voxel, "representative": "mean"}}, **kw)
    want_mean = S.simplify(pv, pf, 2 * voxel, "mean")
    assert again["mesh_vertices"].tobytes() == want_mean[0][0].tobytes() and again["mesh_faces"].tobytes() == want_mean[0][1].tobytes()
    assert again["mesh_info"]["quadric"] == 0 and again["mesh_faces"].tobytes() == f.tobytes()
