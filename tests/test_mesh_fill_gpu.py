"""Mesh hole filling on the MI355X (csrc/mesh_fill.hip, cer-mvs_amd/mesh.py mesh_holes / fill_holes) against the numpy
restatement of tests/mesh_fill_reference.py.  Every comparison is exact: integers as integers, positions as bits, ``info`` as
dictionaries.  The restatement itself is held to hand-written results and to the figures of the analytic meshes in
tests/test_mesh_fill_cpu.py."""
import numpy as np
import pytest
import torch

import mesh_attr_reference as A
import mesh_fill_reference as R
import mesh_smooth_reference as S

pytestmark = pytest.mark.gpu

FIELDS = ("sphere12", "open12", "random")
MAX_EDGES = (3, 8, 64, 1000)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fields():
    """the three small analytic meshes, computed once and left unchanged"""
    return {name: S.field_mesh(name) for name in FIELDS}


@pytest.fixture(scope="module")
def punched24():
    return R.punched_sphere(24, 9.3, 12)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev_fill(dev, vertices, faces, max_edges, colors=None):
    from cer_mvs_amd import mesh as ME
    v, f = R.as_vertices(vertices), R.as_faces(faces)
    info = {}
    out = ME.fill_holes(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), max_edges,
                        colors=None if colors is None else torch.from_numpy(colors).to(dev), info=info)
    ov, of, hole, oc = out
    assert ov.dtype == torch.float32 and of.dtype == torch.int32 and hole.dtype == torch.int32 and all(a.is_cuda for a in (ov, of, hole))
    assert ov.dim() == 2 and ov.shape[1] == 3 and of.dim() == 2 and of.shape[1] == 3 and hole.shape == (of.shape[0],)
    assert (oc is None) == (colors is None) and (oc is None or (oc.dtype == torch.uint8 and oc.is_cuda and oc.shape == ov.shape))
    assert tuple(info) == R.INFO_KEYS and all(type(x) is int for x in info.values())
    return tuple(None if a is None else a.cpu().numpy() for a in out), info


def check_fill(dev, vertices, faces, max_edges, what="", colors=None, with_holes=True):
    """mesh_holes and all four results of fill_holes on the device against the restatement -> (the device's results, info)"""
    from cer_mvs_amd import mesh as ME
    v, f = R.as_vertices(vertices), R.as_faces(faces)
    key = (what, max_edges)
    if with_holes:
        fd, vd = torch.from_numpy(f).to(dev), torch.from_numpy(v).to(dev)
        for given, ref in ((vd, R.mesh_holes(f, len(v), max_edges, v)), (None, R.mesh_holes(f, len(v), max_edges))):
            heads, lens = ME.mesh_holes(fd, len(v), max_edges, vertices=given)
            assert heads.dtype == lens.dtype == torch.int32 and heads.is_cuda and lens.is_cuda and heads.dim() == 1, key
            assert heads.cpu().numpy().tolist() == ref[0].tolist() and lens.cpu().numpy().tolist() == ref[1].tolist(), key
    got, ginfo = dev_fill(dev, v, f, max_edges, colors)
    want, winfo = R.fill(v, f, max_edges, colors)
    assert ginfo == winfo, (key, ginfo, winfo)
    assert got[0].shape == want[0].shape and np.array_equal(bits(got[0]), bits(want[0])), key
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), key
    assert (got[3] is None and want[3] is None) or np.array_equal(got[3], want[3]), key
    assert got[0][:len(v)].tobytes() == v.tobytes() and got[1][:len(f)].tobytes() == f.tobytes() and (got[2][:len(f)] == -1).all(), key
    return got, ginfo


# ---------------------------------------------------------------- hand-made meshes
def test_fill_hand_made_and_empty(dev):
    (v, f, hole, c), info = check_fill(dev, np.zeros((0, 3), np.float32), [], 8, "nv = 0", colors=np.zeros((0, 3), np.uint8))
    assert v.shape == (0, 3) and f.shape == (0, 3) and hole.shape == (0,) and c.shape == (0, 3)
    assert info == dict(holes=0, added_vertices=0, added_faces=0, pinched_vertices=0, boundary_edges_before=0)
    lone = np.arange(12, dtype=np.float32).reshape(4, 3)
    (v, f, _, _), info = check_fill(dev, lone, [], 8, "nf = 0 with nv > 0")
    assert v.tobytes() == lone.tobytes() and f.shape == (0, 3) and info["holes"] == 0
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    (v, f, hole, _), info = check_fill(dev, tri, S.TRIANGLE, 3, "one triangle")
    assert f.tolist() == [[0, 1, 2], [0, 2, 1]] and hole.tolist() == [-1, 0] and len(v) == 3                 # the two-faced closed pillow
    assert info == dict(holes=1, added_vertices=0, added_faces=1, pinched_vertices=0, boundary_edges_before=3)
    pv = np.array(R.PAIR_VERTICES, np.float32)
    col = np.array([[10, 0, 255], [11, 1, 255], [12, 2, 254], [14, 0, 255]], np.uint8)
    (v, f, hole, c), info = check_fill(dev, pv, R.PAIR, 4, "two triangles", colors=col)
    p = pv.astype(np.float64)
    centre = (((((0.0 + p[0]) + p[1]) + p[3]) + p[2]) / 4.0).astype(np.float32)
    assert f[2:].tolist() == [[1, 0, 4], [3, 1, 4], [2, 3, 4], [0, 2, 4]] and hole.tolist() == [-1, -1, 0, 0, 0, 0]
    assert v[4].tobytes() == centre.tobytes() and c[4].tolist() == [11, 0, 254]
    assert info == dict(holes=1, added_vertices=1, added_faces=4, pinched_vertices=0, boundary_edges_before=4)
    assert check_fill(dev, pv, R.PAIR, 3, "two triangles, max_edges 3")[1]["holes"] == 0
    B = float(np.float32(1e17))
    odd = np.array([[B, 0, 0], [1.0, 0, 0], [-B, 0, 0], [0.25, 0, 0]], np.float32)                              # the sum runs in cycle order
    assert check_fill(dev, odd, R.PAIR, 8, "order of the sum")[0][0][4, 0] == 0.0
    for faces, nv, pinched in ((R.PAIR_OPPOSITE, 4, 2), (R.FAN_OF_THREE, 5, 2), (R.BOW_TIE, 5, 1)):
        (v, f, _, _), info = check_fill(dev, np.arange(3 * nv, dtype=np.float32).reshape(nv, 3), faces, 1000, str(faces))
        assert len(v) == nv and f.tolist() == faces and info["holes"] == 0 and info["pinched_vertices"] == pinched
    tet = np.array(S.TETRAHEDRON_VERTICES, np.float32)
    (v, f, _, _), info = check_fill(dev, tet, S.TETRAHEDRON, 64, "tetrahedron")
    assert f.tolist() == S.TETRAHEDRON and info == dict(holes=0, added_vertices=0, added_faces=0, pinched_vertices=0, boundary_edges_before=0)
    (_, f, hole, _), info = check_fill(dev, np.zeros((7, 3), np.float32), [[3, 4, 5], [0, 1, 2]], 3, "two triangles apart, an unreferenced vertex")
    assert f[2:].tolist() == [[0, 2, 1], [3, 5, 4]] and hole.tolist() == [-1, -1, 0, 1] and info["holes"] == 2
    bad = pv.copy()
    bad[3, 1] = np.nan                                                                                       # a planted NaN on the loop
    (v, f, _, _), info = check_fill(dev, bad, R.PAIR, 8, "planted NaN")
    assert len(v) == 4 and len(f) == 2 and info["holes"] == 0 and info["boundary_edges_before"] == 4
    bad[3, 1] = np.inf
    assert check_fill(dev, bad, R.PAIR, 8, "planted inf")[1]["holes"] == 0


# ---------------------------------------------------------------- the fields
FIGURES = {"open12": {3: 0, 8: 0, 64: 1, 1000: 1}, "random": {3: 0, 8: 4, 64: 7, 1000: 9}, "sphere12": {3: 0, 8: 0, 64: 0, 1000: 0}}


@pytest.mark.parametrize("name", FIELDS)
def test_fill_equals_the_restatement_on_the_fields(dev, fields, name):
    from cer_mvs_amd import mesh as ME
    v, f, _ = fields[name]
    col = R.random_colors(len(v))
    for max_edges in MAX_EDGES:
        (ov, of, hole, oc), info = check_fill(dev, v, f, max_edges, name, colors=col)
        assert info["holes"] == FIGURES[name][max_edges] and info["pinched_vertices"] == (6 if name == "random" else 0)
        report = ME.mesh_topology(torch.from_numpy(of).to(dev), len(ov))
        assert report == S.topology(of, len(ov))                                                  # the report of a result: the restatement's
        assert report["boundary_edges"] == info["boundary_edges_before"] - int(R.mesh_holes(f, len(v), max_edges, v)[1].sum())     # all interior now
    (ov, of, _, _), _ = check_fill(dev, v, f, 64, name, with_holes=False)                         # without colours
    again, _ = dev_fill(dev, v, f, 64, colors=col)
    first, _ = dev_fill(dev, v, f, 64, colors=col)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))                          # two runs: the same bytes
    if name == "open12":
        assert (len(ov), len(of)) == (591, 1178) and ME.mesh_topology(torch.from_numpy(of).to(dev), 591)["closed"]
    if name == "random":
        assert (len(ov), len(of)) == (1127, 1776)
    if name == "sphere12":
        assert of.tobytes() == f.tobytes() and ov.tobytes() == v.tobytes()


def test_fill_of_a_renumbered_open_sphere(dev, fields):
    """the 12^3 open sphere renumbered by a seeded permutation with shuffled faces, against the restatement of the permuted input"""
    v, f, _ = fields["open12"]
    v2, f2, new_of_old = S.renumbered(v, f, seed=3)
    for max_edges in (8, 53, 54, 64):                                                             # the loop has 54 edges: the threshold on both sides
        (pv, pf, _, _), pinfo = check_fill(dev, v, f, max_edges, "plain")
        (rv, rf, _, _), rinfo = check_fill(dev, v2, f2, max_edges, "renumbered", colors=R.random_colors(len(v2)))
        assert pinfo == rinfo and pinfo["holes"] == (1 if max_edges >= 54 else 0)
    assert np.abs(pv[590].astype(np.float64) - rv[590]).max() < 1e-5                              # the sum starts elsewhere: close, not bit-equal
    assert sorted(new_of_old[pf[1124:, :2]].tolist()) == sorted(rf[1124:, :2].tolist())           # the same fan on the same rim


# ---------------------------------------------------------------- punched spheres
def test_fill_closes_the_punched_sphere(dev, punched24):
    """the quality bar of the issue on the device's own output: the signed volume within 0.5 % of the unpunched mesh's (the restatement
    measured 3347.03 against 3349.79: 0.08 %) - a cap that faces inward or is missing would show"""
    from cer_mvs_amd import mesh as ME
    (v, f), (wv, wf) = punched24
    assert (len(v), len(f)) == (4713, 9252)
    before = ME.mesh_topology(torch.from_numpy(f).to(dev), len(v))
    assert before == S.topology(f, len(v)) and before["boundary_loops"] == 9 and before["euler"] == -7
    col = R.random_colors(len(v))
    (ov, of, _, _), info = check_fill(dev, v, f, 16, "punched 24^3", colors=col)
    assert info["holes"] == 4
    (ov, of, hole, oc), info = check_fill(dev, v, f, 64, "punched 24^3", colors=col)
    assert info == dict(holes=9, added_vertices=9, added_faces=188, pinched_vertices=0, boundary_edges_before=188) and (len(ov), len(of)) == (4722, 9440)
    od, fd = torch.from_numpy(ov).to(dev), torch.from_numpy(of).to(dev)
    report = ME.mesh_topology(fd, len(ov))
    assert report == S.topology(of, len(ov))
    assert report["closed"] and report["oriented"] and report["euler"] == 2 and report["nonmanifold_edges"] == 0 and report["boundary_loops"] == 0
    vol, whole = S.signed_volume(ov, of), S.signed_volume(wv, wf)
    print(f"punched 24^3 sphere on the device, max_edges = 64: signed volume {vol:.2f} against {whole:.2f} unpunched ({abs(vol - whole) / whole:.4%})")
    assert abs(vol - whole) <= 0.005 * whole
    # what runs next on a filled mesh: finite, and bit-equal to the restatements
    normals = ME.vertex_normals(od, fd).cpu().numpy()
    assert np.isfinite(normals).all() and np.array_equal(bits(normals), bits(A.vertex_normals(ov, of)))
    sinfo = {}
    smoothed = ME.smooth_mesh(od, fd, 3, info=sinfo).cpu().numpy()
    want, winfo = S.smooth(ov, of, 3)
    assert np.isfinite(smoothed).all() and np.array_equal(bits(smoothed), bits(want)) and sinfo == winfo and sinfo["frozen_boundary"] == 0


def test_fill_many_holes_across_blocks(dev):
    """the 40^3 sphere punched at 60 nodes: 12 752 vertices in 50 blocks of 256, 50 loops of which 3 run through a pinched vertex and stay"""
    (v, f), _ = R.punched_sphere(40, 15.5, 60)
    assert (len(v), len(f)) == (12752, 24560)
    before = S.topology(f, len(v))
    assert before["boundary_loops"] == 50 and int((R.next_table(f, len(v)) == -2).sum()) == 3
    col = R.random_colors(len(v))
    for max_edges, holes in ((16, 15), (24, 43), (64, 47)):
        (ov, of, hole, _), info = check_fill(dev, v, f, max_edges, "punched 40^3", colors=col)
        assert info["holes"] == holes and info["pinched_vertices"] == 3 and info["boundary_edges_before"] == before["boundary_edges"]
    blocks = (R.mesh_holes(f, len(v), 64, v)[0] // 256).tolist()
    assert len(set(blocks)) >= 10 and len(blocks) > len(set(blocks))                              # heads in many blocks, and more than one in some
    assert (len(ov), len(of)) == (12799, 25500) and S.topology(of, len(ov))["boundary_loops"] == 3


def test_fill_refuses_bad_arguments_on_the_device(dev, fields):
    from cer_mvs_amd import mesh as ME
    sv, sf, _ = fields["open12"]
    v, f = torch.from_numpy(sv).to(dev), torch.from_numpy(sf).to(dev)
    with pytest.raises(ValueError, match="indices"):
        ME.fill_holes(v[:500], f, 8)
    with pytest.raises(ValueError, match="indices"):
        ME.mesh_holes(f, 500, 8)
    with pytest.raises(ValueError, match="one device"):
        ME.fill_holes(v, f.cpu(), 8)
    with pytest.raises(ValueError, match="one device"):
        ME.mesh_holes(f, len(sv), 8, vertices=v.cpu())
    with pytest.raises(ValueError, match="max_edges"):
        ME.fill_holes(v, f, 2)
    heads, lens = ME.mesh_holes(f, len(sv), 1 << 40)                                              # held to a C int, not refused
    assert lens.tolist() == [54]


# ---------------------------------------------------------------- the tool
def test_mesh_fill_tool(dev, fields, tmp_path, monkeypatch, capsys):
    """tools/mesh_fill.py, run in this process"""
    import importlib.util
    import json
    import os
    from conftest import REPO
    from cer_mvs_amd import mesh as ME
    spec = importlib.util.spec_from_file_location("mesh_fill_tool", os.path.join(REPO, "tools", "mesh_fill.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    v, f, _ = fields["random"]
    col = R.random_colors(len(v))
    (wv, wf, _, wc), winfo = R.fill(v, f, 64, col)
    src, dst = tmp_path / "in.ply", tmp_path / "out.ply"
    for normals_in, colors_in in ((True, True), (False, True), (False, False)):
        ME.write_mesh_ply(src, v, f, normals=A.vertex_normals(v, f) if normals_in else None, colors=col if colors_in else None)
        monkeypatch.setattr("sys.argv", ["mesh_fill.py", str(src), str(dst), "--max-edges", "64"])
        tool.main()
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert line["vertices"] == len(wv) and line["faces"] == len(wf) and {k: line[k] for k in winfo} == winfo
        rv, rf, rn, rc = ME.read_mesh_ply(dst, attributes=True)
        assert np.array_equal(bits(rv), bits(wv)) and np.array_equal(rf, wf)
        assert (rc is not None) == colors_in and (rc is None or np.array_equal(rc, wc))           # colours carried through, the centres' added
        assert (rn is not None) == normals_in and (rn is None or np.array_equal(bits(rn), bits(A.vertex_normals(wv, wf))))     # normals recomputed


# ---------------------------------------------------------------- chain
SAME_KEYS = ("xyz", "rgb", "masks", "depth_est")
PLAIN_INFO = {"grid", "trunc", "nv", "nf", "observed"}


def test_reconstruct_scan_fill_holes(dev, tmp_path):
    import test_reconstruct_gpu as TR
    from cer_mvs_amd import mesh as ME
    from cer_mvs_amd.scan import reconstruct_scan
    images, poses, intr, scales = TR._scan(128, 160)
    model = TR._model(dev)
    args = (model, images, poses, intr, TR.NAMES, TR.PAIRS, scales)
    kw = dict(num_frames=TR.NF, streams=2)
    plain_dir, fill_dir = tmp_path / "plain", tmp_path / "fill"
    plain_dir.mkdir()
    fill_dir.mkdir()
    plain = reconstruct_scan(*args, plain_dir, mesh={"resolution": 48, "topology": True}, **kw)
    assert set(plain["mesh_info"]) == PLAIN_INFO | {"topology"}                                  # without the new key: no new key
    out = reconstruct_scan(*args, fill_dir, mesh={"resolution": 48, "fill_holes": 32, "topology": True}, **kw)
    for key in SAME_KEYS:                                                                        # cloud, masks and depths: byte-equal to the plain run
        assert out[key].dtype == plain[key].dtype and out[key].tobytes() == plain[key].tobytes(), key
    assert (fill_dir / "result.ply").read_bytes() == (plain_dir / "result.ply").read_bytes()
    pv, pf = plain["mesh_vertices"], plain["mesh_faces"]
    (dv, df, _, _), dinfo = check_fill(dev, pv, pf, 32, "the scan's mesh", with_holes=False)
    v, f, info = out["mesh_vertices"], out["mesh_faces"], out["mesh_info"]
    assert v.dtype == np.float32 and f.dtype == np.int32 and np.array_equal(bits(v), bits(dv)) and np.array_equal(f, df)
    assert set(info) - PLAIN_INFO == {"filled", "topology"} and info["filled"] == dinfo and (info["nv"], info["nf"]) == (len(dv), len(df))
    assert {k: info[k] for k in PLAIN_INFO - {"nv", "nf"}} == {k: plain["mesh_info"][k] for k in PLAIN_INFO - {"nv", "nf"}}
    assert info["topology"] == S.topology(f, len(v)) and dinfo["holes"] >= 1
    assert info["topology"]["boundary_loops"] == plain["mesh_info"]["topology"]["boundary_loops"] - dinfo["holes"]
    print(f"reconstruct_scan fill_holes = 32: {dinfo}; loops {plain['mesh_info']['topology']['boundary_loops']} -> {info['topology']['boundary_loops']}")
    rv, rf = ME.read_mesh_ply(fill_dir / "result_mesh.ply")
    assert np.array_equal(bits(rv), bits(v)) and np.array_equal(rf, f)
    # "fill_holes" with "smooth": the two calls in that order
    both = reconstruct_scan(*args, None, write=False, mesh={"resolution": 48, "fill_holes": 32, "smooth": 3}, **kw)
    want, winfo = S.smooth(dv, df, 3)
    assert np.array_equal(bits(both["mesh_vertices"]), bits(want)) and np.array_equal(both["mesh_faces"], df)
    assert both["mesh_info"]["filled"] == dinfo and both["mesh_info"]["smoothed"] == winfo
    assert winfo["frozen_boundary"] < S.smooth(pv, pf, 1)[1]["frozen_boundary"]                  # fewer vertices frozen on a boundary than before
