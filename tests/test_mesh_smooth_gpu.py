"""Mesh edges, the topology report and Taubin smoothing on the MI355X (csrc/mesh.hip, cer-mvs_amd/mesh.py mesh_edges / edge_table /
mesh_topology / smooth_mesh) against the numpy restatement of tests/mesh_smooth_reference.py.  Every comparison is exact:
integers as integers, positions as bits, the report and the info figures as dictionaries.  The restatement itself is held to hand-written
results and to the figures of the analytic meshes in tests/test_mesh_smooth_cpu.py."""
import numpy as np
import pytest
import torch

import mesh_attr_reference as A
import mesh_reference as M
import mesh_smooth_reference as R

pytestmark = pytest.mark.gpu

INFO_KEYS = {"moved", "frozen_boundary", "steps", "edges"}
FIELDS = ("sphere12", "open12", "random")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fields():
    """the three small analytic meshes, computed once and left unchanged"""
    return {name: R.field_mesh(name) for name in FIELDS}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_edges(dev, faces, nv, what=""):
    """mesh_edges, edge_table and mesh_topology on the device against the restatement -> the report"""
    from cer_mvs_amd import mesh as ME
    f = torch.from_numpy(R.as_faces(faces)).to(dev)
    out = ME.mesh_edges(f, nv)
    names = ("nbr_starts", "nbrs", "along", "against")
    want = R.mesh_edges(faces, nv)
    for a, b, name in zip(out, want, names):
        assert a.dtype == torch.int32 and a.is_cuda and a.dim() == 1, (what, name)
        assert a.cpu().numpy().tolist() == b.tolist(), (what, name)
    assert out[0].shape[0] == nv + 1 and out[1].shape[0] % 2 == 0
    table = ME.edge_table(*out)
    for a, b, name in zip(table, R.edge_table(faces, nv), ("lo", "hi", "n_lo_hi", "n_hi_lo")):
        assert a.dtype == torch.int32 and a.cpu().numpy().tolist() == b.tolist(), (what, name)
    report = ME.mesh_topology(f, nv)
    ref = R.topology(faces, nv)
    assert tuple(report) == R.TOPOLOGY_KEYS and report == ref, (what, report, ref)
    assert all(type(report[k]) is type(ref[k]) for k in report), what
    return report


def dev_smooth(dev, vertices, faces, iterations, **kw):
    from cer_mvs_amd import mesh as ME
    v, f = R.as_vertices(vertices), R.as_faces(faces)
    info = {}
    out = ME.smooth_mesh(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), iterations, info=info, **kw)
    assert out.dtype == torch.float32 and out.is_cuda and tuple(out.shape) == v.shape and set(info) == INFO_KEYS
    return out.cpu().numpy(), info


def check_smooth(dev, vertices, faces, iterations, what="", **kw):
    got, ginfo = dev_smooth(dev, vertices, faces, iterations, **kw)
    want, winfo = R.smooth(vertices, faces, iterations, **kw)
    assert np.array_equal(bits(got), bits(want)), (what, iterations, kw, int((bits(got) != bits(want)).any(1).sum()))
    assert ginfo == winfo, (what, iterations, kw)
    return got, ginfo


# ---------------------------------------------------------------- edges and the report
def test_edges_and_report_equal_the_restatement_on_hand_made_meshes(dev):
    for name, (faces, nv, want) in R.hand_made().items():
        report = check_edges(dev, faces, nv, name)
        assert {k: report[k] for k in want} == want, name                                   # and what was written out by hand
    report = check_edges(dev, [], 4, "nf = 0 with nv > 0")
    assert report["unreferenced_vertices"] == 4 and report["edges"] == 0 and report["euler"] == 0 and not report["closed"]
    check_edges(dev, [[1, 1, 1], [3, 3, 0]], 4, "degenerate faces only, and one edge from one of them")


@pytest.mark.parametrize("name", FIELDS)
def test_edges_and_report_of_the_fields(dev, fields, name):
    v, f, _ = fields[name]
    report = check_edges(dev, f, len(v), name)
    print(name, report)
    figures = {"sphere12": (970, 1936, 2904, 0, 0, 2, 0), "open12": (590, 1124, 1713, 54, 54, 1, 1), "random": (1120, 1676, 2839, 650, None, None, None)}[name]
    got = tuple(report[k] for k in ("vertices", "faces", "edges", "boundary_edges", "boundary_vertices", "euler", "boundary_loops"))
    assert all(w is None or g == w for g, w in zip(got, figures)), (got, figures)


def test_edges_of_a_renumbered_sphere(dev, fields):
    """the 12^3 sphere renumbered by a seeded permutation with shuffled faces, against the restatement of the permuted input"""
    v, f, _ = fields["sphere12"]
    v2, f2, new_of_old = R.renumbered(v, f, seed=3)
    plain = check_edges(dev, f, len(v), "plain")
    assert check_edges(dev, f2, len(v2), "renumbered") == plain                              # the report does not depend on the numbering
    for kw in (dict(method="taubin"), dict(method="laplacian", boundary="free")):
        a, ainfo = check_smooth(dev, v, f, 3, "plain", **kw)
        b, binfo = check_smooth(dev, v2, f2, 3, "renumbered", **kw)
        assert ainfo == binfo and np.abs(a.astype(np.float64) - b[new_of_old]).max() < 1e-5  # sums in another order: close, not bit-equal


# ---------------------------------------------------------------- smoothing
@pytest.mark.parametrize("name", FIELDS)
def test_smooth_equals_the_restatement(dev, fields, name):
    v, f, _ = fields[name]
    on_boundary = R.boundary_vertices(f, len(v))
    for method in R.METHODS:
        for boundary in R.BOUNDARIES:
            for iterations in (1, 3, 10):
                out, info = check_smooth(dev, v, f, iterations, name, method=method, boundary=boundary)
                assert info["steps"] == iterations * (2 if method == "taubin" else 1)
                if boundary == "fixed":
                    assert np.array_equal(bits(out[on_boundary]), bits(v[on_boundary])) and info["frozen_boundary"] == int(on_boundary.sum())
    if name == "open12":
        _, info = dev_smooth(dev, v, f, 3)
        assert info == dict(moved=536, frozen_boundary=54, steps=6, edges=1713)
        _, info = dev_smooth(dev, v, f, 3, boundary="free")
        assert info == dict(moved=590, frozen_boundary=0, steps=6, edges=1713)
    out, _ = check_smooth(dev, v, f, 2, name, lam=0.33, mu=-0.34)                            # other weights
    again, _ = dev_smooth(dev, v, f, 2, lam=0.33, mu=-0.34)
    assert again.tobytes() == out.tobytes()                                                  # two runs: the same bytes


def test_smooth_hand_made_and_empty(dev):
    tet = np.array(R.TETRAHEDRON_VERTICES, np.float32)
    out, info = check_smooth(dev, tet, R.TETRAHEDRON, 1, "tetrahedron", method="laplacian", lam=1.0)
    p = tet.astype(np.float64)
    others = [[j for j in range(4) if j != i] for i in range(4)]                             # ascending: the contract's order
    want = np.stack([(((0.0 + p[a]) + p[b]) + p[c]) / 3.0 for a, b, c in others])           # the mean of the other three
    assert np.array_equal(bits(out), bits((p + 1.0 * (want - p)).astype(np.float32))) and info == dict(moved=4, frozen_boundary=0, steps=1, edges=6)
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    out, info = check_smooth(dev, tri, R.TRIANGLE, 3, "triangle, fixed")
    assert out.tobytes() == tri.tobytes() and info["moved"] == 0
    out, _ = check_smooth(dev, tri, R.TRIANGLE, 1, "triangle, free", method="laplacian", boundary="free")
    assert out.tolist() == [[0.25, 0.25, 0.0], [0.5, 0.25, 0.0], [0.25, 0.5, 0.0]]
    out, info = dev_smooth(dev, [], [], 2)                                                   # nv = 0
    assert out.shape == (0, 3) and info == dict(moved=0, frozen_boundary=0, steps=4, edges=0)
    lone = np.arange(12, dtype=np.float32).reshape(4, 3)
    out, info = check_smooth(dev, lone, [], 2, "nf = 0 with nv > 0")                         # no neighbour: nothing moves
    assert out.tobytes() == lone.tobytes() and info == dict(moved=0, frozen_boundary=0, steps=4, edges=0)


def test_smooth_with_planted_non_finite_vertices(dev, fields):
    sv, sf, _ = fields["sphere12"]
    v = sv.copy()
    planted = [0, 17, 400, 5, 969]
    v[[0, 17, 400], [0, 1, 2]] = np.nan
    v[[5, 969], [2, 0]] = [np.inf, -np.inf]
    starts, nbrs, _, _ = R.mesh_edges(sf, len(v))
    around = np.setdiff1d(np.concatenate([nbrs[starts[i]:starts[i + 1]] for i in planted]), planted)
    for kw in (dict(method="taubin"), dict(method="laplacian"), dict(method="taubin", boundary="free")):
        for iterations in (1, 10):
            out, info = check_smooth(dev, v, sf, iterations, "planted", **kw)
            assert np.array_equal(bits(out[planted]), bits(v[planted])) and info["moved"] == len(v) - len(planted)
            rest = np.setdiff1d(np.arange(len(v)), planted)
            assert np.isfinite(out[rest]).all()                                              # no NaN spreads, not even to the neighbours
            assert (bits(out[around]) != bits(v[around])).any(1).all()                       # which move, on the mean of their finite neighbours
    none = np.full((4, 3), np.nan, np.float32)
    none[1] = [np.inf, 0.0, 0.0]
    out, info = check_smooth(dev, none, R.TETRAHEDRON, 3, "no finite vertex")
    assert np.array_equal(bits(out), bits(none)) and info["moved"] == 0
    alone = np.array(R.TETRAHEDRON_VERTICES, np.float32)
    alone[1:] = np.nan                                                                       # one finite vertex without a finite neighbour
    out, info = check_smooth(dev, alone, R.TETRAHEDRON, 3, "one finite vertex")
    assert np.array_equal(bits(out), bits(alone)) and info["moved"] == 0


def test_edges_and_smoothing_across_compaction_tiles(dev):
    """65 x 64 x 64 nodes: 33 266 vertices and 399 168 keys - about 195 tiles of 2048 in the compaction"""
    from cer_mvs_amd import mesh as ME
    tsdf, weight, grid, centre = M.sphere_field((65, 64, 64), 24.3)
    v, f = M.extract_mesh(tsdf, weight, grid)
    assert len(v) == 33266 and len(f) == 66528 and 6 * len(f) > 100 * ME.MESH_TILE
    report = check_edges(dev, f, len(v), "65x64x64 sphere")
    print("65x64x64 sphere", report)
    assert report["edges"] == 99792 and report["closed"] and report["oriented"] and report["euler"] == 2
    out, info = check_smooth(dev, v, f, 2, "65x64x64 sphere")
    assert info == dict(moved=33266, frozen_boundary=0, steps=4, edges=99792)
    again, _ = dev_smooth(dev, v, f, 2)
    assert again.tobytes() == out.tobytes()                                                  # two runs: the same bytes
    normals = ME.vertex_normals(torch.from_numpy(out).to(dev), torch.from_numpy(f).to(dev)).cpu().numpy()
    assert np.isfinite(normals).all() and np.array_equal(bits(normals), bits(A.vertex_normals(out, f)))


def test_smooth_denoises_on_the_device(dev):
    """the quality bars of the issue, on the device's own output (which the restatement equals bit for bit)"""
    v, f, centre = R.field_mesh("sphere24")
    noisy = R.radial_noise(v, centre, 9.3)
    d0, vol0 = R.sphere_distance_mean(noisy, centre, 9.3), R.signed_volume(noisy, f)
    out, info = dev_smooth(dev, noisy, f, 10)
    d1, vol1 = R.sphere_distance_mean(out, centre, 9.3), R.signed_volume(out, f)
    lap, _ = dev_smooth(dev, noisy, f, 20, method="laplacian")
    vol2 = R.signed_volume(lap, f)
    print(f"24^3 sphere, noisy: mean distance {d0:.4f}, volume {vol0:.2f}; taubin x 10: {d1:.4f}, {vol1:.2f} (ratio {d1 / d0:.3f}); laplacian x 20: volume {vol2:.2f}")
    assert d1 <= 0.5 * d0 and abs(vol1 - vol0) <= 0.01 * vol0 and vol2 < 0.96 * vol0
    assert info == dict(moved=4848, frozen_boundary=0, steps=20, edges=14538)


def test_smooth_refuses_bad_arguments_on_the_device(dev, fields):
    from cer_mvs_amd import mesh as ME
    sv, sf, _ = fields["sphere12"]
    v, f = torch.from_numpy(sv).to(dev), torch.from_numpy(sf).to(dev)
    with pytest.raises(ValueError, match="indices"):
        ME.smooth_mesh(v[:900], f, 1)
    with pytest.raises(ValueError, match="indices"):
        ME.mesh_edges(f, 900)
    with pytest.raises(ValueError, match="one device"):
        ME.smooth_mesh(v, f.cpu(), 1)
    with pytest.raises(ValueError, match="iterations"):
        ME.smooth_mesh(v, f, 0)


# ---------------------------------------------------------------- tools
def _tool(name):
    import importlib.util
    import os
    from conftest import REPO
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(REPO, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_mesh_smooth_and_topology_tools(dev, fields, tmp_path, monkeypatch, capsys):
    """tools/mesh_smooth.py and tools/mesh_topology.py, run in this process"""
    import json
    from cer_mvs_amd import mesh as ME
    v, f, _ = fields["open12"]
    col = np.random.default_rng(4).integers(0, 256, size=(len(v), 3)).astype(np.uint8)
    smooth_tool, topology_tool = _tool("mesh_smooth"), _tool("mesh_topology")
    src, dst = tmp_path / "in.ply", tmp_path / "out.ply"
    want, winfo = R.smooth(v, f, 2, "laplacian", lam=0.4, boundary="free")
    for normals_in, flag, normals_out in ((True, [], True), (False, [], False), (False, ["--normals"], True)):
        ME.write_mesh_ply(src, v, f, normals=A.vertex_normals(v, f) if normals_in else None, colors=col)
        monkeypatch.setattr("sys.argv", ["mesh_smooth.py", str(src), str(dst), "--iterations", "2", "--method", "laplacian", "--lam", "0.4",
                                         "--boundary", "free"] + flag)
        smooth_tool.main()
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert line["vertices"] == len(v) and line["faces"] == len(f) and {k: line[k] for k in winfo} == winfo
        rv, rf, rn, rc = ME.read_mesh_ply(dst, attributes=True)
        assert np.array_equal(bits(rv), bits(want)) and np.array_equal(rf, f) and np.array_equal(rc, col)      # colours carried through
        assert (rn is not None) == normals_out and (rn is None or np.array_equal(bits(rn), bits(A.vertex_normals(want, f))))
    ME.write_mesh_ply(src, v, f)
    monkeypatch.setattr("sys.argv", ["mesh_smooth.py", str(src), str(dst), "--iterations", "3"])                # the defaults: Taubin, fixed
    smooth_tool.main()
    capsys.readouterr()
    assert np.array_equal(bits(ME.read_mesh_ply(dst)[0]), bits(R.smooth(v, f, 3)[0]))
    monkeypatch.setattr("sys.argv", ["mesh_topology.py", str(src)])
    topology_tool.main()
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == R.topology(f, len(v))


# ---------------------------------------------------------------- chain
SAME_KEYS = ("xyz", "rgb", "masks", "depth_est")
PLAIN_INFO = {"grid", "trunc", "nv", "nf", "observed"}


def test_reconstruct_scan_smooth_and_topology(dev, tmp_path):
    import mesh_simplify_reference as S
    import test_reconstruct_gpu as TR
    from cer_mvs_amd import mesh as ME
    from cer_mvs_amd.scan import reconstruct_scan
    images, poses, intr, scales = TR._scan(128, 160)
    model = TR._model(dev)
    args = (model, images, poses, intr, TR.NAMES, TR.PAIRS, scales)
    kw = dict(num_frames=TR.NF, streams=2)
    plain_dir, smooth_dir = tmp_path / "plain", tmp_path / "smooth"
    plain_dir.mkdir()
    smooth_dir.mkdir()
    plain = reconstruct_scan(*args, plain_dir, mesh={"resolution": 48}, **kw)
    assert set(plain["mesh_info"]) == PLAIN_INFO                                                 # without the new keys: no new key
    out = reconstruct_scan(*args, smooth_dir, mesh={"resolution": 48, "smooth": 3, "topology": True}, **kw)
    for key in SAME_KEYS:                                                                        # cloud, masks and depths: byte-equal to the plain run
        assert out[key].dtype == plain[key].dtype and out[key].tobytes() == plain[key].tobytes(), key
    assert (smooth_dir / "result.ply").read_bytes() == (plain_dir / "result.ply").read_bytes()
    pv, pf = plain["mesh_vertices"], plain["mesh_faces"]
    direct, dinfo = dev_smooth(dev, pv, pf, 3)
    want, winfo = R.smooth(pv, pf, 3)
    assert np.array_equal(bits(direct), bits(want)) and dinfo == winfo
    v, f, info = out["mesh_vertices"], out["mesh_faces"], out["mesh_info"]
    assert v.dtype == np.float32 and f.dtype == np.int32 and np.array_equal(bits(v), bits(want)) and f.tobytes() == pf.tobytes()
    assert set(info) - PLAIN_INFO == {"smoothed", "topology"} and info["smoothed"] == winfo and {k: info[k] for k in PLAIN_INFO} == plain["mesh_info"]
    report = ME.mesh_topology(torch.from_numpy(f).to(dev), len(v))
    assert info["topology"] == report == R.topology(f, len(v))
    print(f"reconstruct_scan smooth = 3: {info['smoothed']}, {report}")
    rv, rf = ME.read_mesh_ply(smooth_dir / "result_mesh.ply")
    assert np.array_equal(bits(rv), bits(v)) and np.array_equal(rf, f)
    # "smooth" with "simplify": the two calls in that order
    both = reconstruct_scan(*args, None, write=False, mesh={"resolution": 48, "smooth": {"iterations": 2, "boundary": "free"}, "simplify": 2,
                                                             "topology": True}, **kw)
    voxel = plain["mesh_info"]["grid"].voxel
    smoothed, sinfo = R.smooth(pv, pf, 2, boundary="free")
    (wv, wf, _, _), simplified_info = S.simplify(smoothed, pf, 2 * voxel, "quadric")
    assert np.array_equal(bits(both["mesh_vertices"]), bits(wv)) and np.array_equal(both["mesh_faces"], wf)
    binfo = both["mesh_info"]
    assert binfo["smoothed"] == sinfo and binfo["simplified_from"] == (len(pv), len(pf)) and {k: binfo[k] for k in simplified_info} == simplified_info
    assert binfo["topology"] == R.topology(wf, len(wv))
