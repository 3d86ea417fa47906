"""Surface normals for point clouds (csrc/cloud_eval.hip grid_normals_kernel, cer-mvs_amd/cloud_eval.py CloudIndex.normals / estimate_normals,
fusion.write_ply / cloud_eval.read_ply with normals), the parts that need no GPU: the entry point of ABI 1150 and its argument
checks in the documented order, the ValueErrors of the Python layer, the PLY round trip with and without normals, and the oracle of
tests/normals_reference.py against cases worked by hand."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import knn_reference as R
import normals_reference as NR
from conftest import REPO

BIG = 1 << 31
NAN, INF = float("nan"), float("inf")
F32 = np.float32


def test_normals_abi_symbol_is_declared_and_bound():
    from cer_mvs_amd import _lib as L
    from cer_mvs_amd import cloud_eval as CE
    hdr = open(os.path.join(REPO, "include", "cer_mvs.h")).read()
    assert "cer_grid_normals_f32" in L.exported_symbols()
    assert "int cer_grid_normals_f32(const void* records, long n, const long long* cell_keys, const long long* cell_start, long ncells" in hdr
    sig, knn = L._SIGNATURES["cer_grid_normals_f32"], L._SIGNATURES["cer_grid_knn_f32"]
    assert sig[0] is L._I and sig[1][:12] == knn[1][:12] and len(sig[1]) == 19 and sig[1][12:] == [L._P] * 7      # knn's head + 6 pointers + stream
    assert L.ABI_VERSION >= 1150
    lib = L.load()                                        # (loads without a GPU; refuses a library that lacks a declared symbol)
    assert lib.cer_abi_version() == L.ABI_VERSION
    assert "ABI 1140" in hdr and "ABI 1150" in hdr
    for word in ("const float* points,", "const float* viewpoints, float* normal, float* curvature, int* count, double* mom, void* stream);"):
        assert word in hdr
    assert len(L.exported_symbols()) >= 96
    assert CE.NORMAL_DEGENERATE == CE.COLLINEAR_RATIO == NR.NORMAL_DEGENERATE == 1e-12


def test_normals_entry_point_refuses_bad_arguments_in_the_documented_order():
    """argument checks run before any launch (the pointers are fake: a launch would fault).  The order is grid_search_rings', as
    cer_grid_knn_f32 passes through it: sizes; frame, reach and k < 1 -> CER_EINVAL; ncells > n and k > CER_KNN_MAX -> CER_ESHAPE; rings ->
    CER_ESHAPE; an empty side -> CER_OK; null pointers (count and points among them; viewpoints, normal, curvature and mom may be null) ->
    CER_EINVAL; alignment -> CER_EALIGN.  Two faults at once: the earlier check answers."""
    from cer_mvs_amd import _lib as L
    lib = L.load()
    fake, null = ctypes.c_void_p(4096), None
    o = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    o_nan = (ctypes.c_double * 3)(0.0, NAN, 0.0)
    no_o = ctypes.POINTER(ctypes.c_double)()
    odd = ctypes.c_void_p(4104)

    def nrm(n=8, nc=3, m=5, rec=fake, ck=fake, cs=fake, org=o, cell=0.5, q=fake, qo=null, k=4, md=1.0, pts=fake, vp=fake, normal=fake, curv=fake,
            count=fake, mom=fake):
        return lib.cer_grid_normals_f32(rec, n, ck, cs, nc, org, cell, q, qo, m, k, md, pts, vp, normal, curv, count, mom, null)
    assert nrm(n=-1) == -1 and nrm(m=-1) == -1 and nrm(nc=-1) == -1
    assert nrm(n=BIG) == -2 and nrm(m=BIG) == -2 and nrm(nc=9) == -2
    assert nrm(org=no_o) == -1 and nrm(org=o_nan) == -1 and nrm(cell=0.0) == -1 and nrm(cell=NAN) == -1
    assert nrm(md=-1.0) == -1 and nrm(md=NAN) == -1
    assert nrm(k=0) == -1 and nrm(k=-3) == -1
    assert nrm(k=33) == -2 and nrm(k=1 << 20) == -2
    for k in (1, 8, 9, 16, 17, 32):                       # every width: the checks pass and an empty side launches nothing
        assert nrm(k=k, m=0) == 0
    assert nrm(md=INF) == -2 and nrm(md=5000.0, cell=1.0) == -2            # more rings than the search enumerates
    assert nrm(m=0) == 0 and nrm(n=0, nc=0) == 0 and nrm(nc=0) == 0
    assert nrm(m=0, rec=null, ck=null, cs=null, q=null, pts=null, vp=null, normal=null, curv=null, count=null, mom=null) == 0
    assert nrm(rec=null) == -1 and nrm(ck=null) == -1 and nrm(cs=null) == -1 and nrm(q=null) == -1
    assert nrm(count=null) == -1 and nrm(pts=null) == -1 and nrm(count=null, vp=null, normal=null, curv=null, mom=null) == -1
    assert nrm(rec=odd) == -3
    # the order: sizes before k, k < 1 (CER_EINVAL) before k > 32's class (CER_ESHAPE: nc > n), both before the empty side and the pointers
    assert nrm(n=BIG, k=0) == -2 and nrm(m=-1, k=33) == -1
    assert nrm(k=0, nc=9) == -1 and nrm(k=0, md=INF) == -1 and nrm(k=0, m=0) == -1 and nrm(k=0, count=null) == -1 and nrm(k=0, pts=null) == -1
    assert nrm(k=33, md=-1.0) == -1 and nrm(k=33, m=0) == -2 and nrm(k=33, count=null) == -2 and nrm(k=33, pts=null) == -2 and nrm(k=33, rec=odd) == -2
    assert nrm(md=INF, m=0) == -2 and nrm(md=INF, count=null) == -2 and nrm(md=INF, pts=null) == -2
    assert nrm(count=null, rec=odd) == -1 and nrm(pts=null, rec=odd) == -1 and nrm(pts=null, m=0) == 0


def test_python_layer_raises_value_errors():
    """``k`` outside 1 .. 32 and bad distances are refused before the tensors are looked at; a tensor that is not on the device is not a
    ValueError but the package's "no CPU fallback\""""
    from cer_mvs_amd import cloud_eval as CE
    from cer_mvs_amd.scan import reconstruct_scan
    index = CE.CloudIndex.__new__(CE.CloudIndex)          # (no GPU here: the checks below come before the index is touched)
    p = torch.zeros(4, 3)
    for k in (0, -1, 33, 100):
        with pytest.raises(ValueError, match="1 .. 32"):
            index.normals(p, k, 0.1)
        with pytest.raises(ValueError, match="1 .. 32"):
            CE.estimate_normals(p, k=k)
    for bad in (-1.0, NAN):
        with pytest.raises(ValueError, match="max_dist"):
            index.normals(p, 4, bad)
        with pytest.raises(ValueError, match="max_dist"):
            CE.estimate_normals(p, max_dist=bad)
    with pytest.raises(ValueError, match="max_dist"):
        CE.estimate_normals(p, max_dist=INF)              # remove_statistical_outliers' rule: finite
    with pytest.raises(ValueError, match="cell"):
        CE.estimate_normals(p, cell=0.0)
    with pytest.raises(RuntimeError, match="CUDA"):
        index.normals(p, 4, 0.1)
    with pytest.raises(RuntimeError, match="CUDA"):
        CE.estimate_normals(p)
    for bad in ("yes", 1, False, {"k": 8, "radius": 0.1}, {"method": "pca"}):
        with pytest.raises(ValueError, match="normals"):
            CE.normals_options(bad)
        with pytest.raises(ValueError, match="normals"):   # ... and reconstruct_scan refuses it before it touches the model or the images
            reconstruct_scan(None, [None], None, None, ["a"], [[0]], [1.0], write=False, normals=bad)
    assert CE.normals_options(True) == {} and CE.normals_options({"k": 8, "max_dist": 0.1, "cell": 0.05}) == {"k": 8, "max_dist": 0.1, "cell": 0.05}
    par = inspect.signature(reconstruct_scan).parameters
    assert par["normals"].default is None and par["clean"].default is None
    par = inspect.signature(CE.CloudIndex.normals).parameters
    assert list(par)[1:] == ["queries", "k", "max_dist", "viewpoints", "sort_queries", "moments"]
    assert par["viewpoints"].default is None and par["sort_queries"].default is True and par["moments"].default is False
    par = inspect.signature(CE.estimate_normals).parameters
    assert list(par) == ["points", "k", "max_dist", "cell", "viewpoints", "info"] and par["k"].default == 20
    from cer_mvs_amd import fusion as FU
    assert inspect.signature(FU.point_cloud).parameters["view_base"].default is False
    assert inspect.signature(FU.write_ply).parameters["normals"].default is None


def _todays_ply(xyz, rgb):
    """the bytes ``fusion.write_ply`` wrote before it took normals, restated"""
    v = np.empty(len(xyz), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    v["x"], v["y"], v["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    v["red"], v["green"], v["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    header = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    return header.encode("ascii") + v.tobytes()


@pytest.mark.parametrize("n", [0, 1, 37])
def test_ply_round_trip_with_and_without_normals(tmp_path, n):
    from cer_mvs_amd.cloud_eval import read_ply
    from cer_mvs_amd.fusion import write_ply
    g = np.random.default_rng(5 + n)
    xyz = g.standard_normal((n, 3)).astype(F32)
    rgb = g.integers(0, 256, (n, 3)).astype(np.uint8)
    nrm = g.standard_normal((n, 3)).astype(F32)
    if n:
        nrm[0] = (0.0, -0.0, NAN)                            # bits travel as they are
    plain, with_n = str(tmp_path / "plain.ply"), str(tmp_path / "normals.ply")
    write_ply(plain, xyz, rgb)
    assert open(plain, "rb").read() == _todays_ply(xyz, rgb)
    write_ply(plain, xyz, rgb, normals=None)
    assert open(plain, "rb").read() == _todays_ply(xyz, rgb)
    x, c = read_ply(plain)
    assert x.tobytes() == xyz.tobytes() and c.tobytes() == rgb.tobytes()
    x, c, k = read_ply(plain, normals=True)
    assert x.tobytes() == xyz.tobytes() and c.tobytes() == rgb.tobytes() and k is None
    write_ply(with_n, xyz, rgb, normals=nrm)
    raw = open(with_n, "rb").read()
    head = raw[:raw.index(b"end_header\n")].decode("ascii").split("\n")
    assert [ln.split()[1:] for ln in head if ln.startswith("property")] == [["float", "x"], ["float", "y"], ["float", "z"], ["float", "nx"],
                                                                             ["float", "ny"], ["float", "nz"], ["uchar", "red"],
                                                                             ["uchar", "green"], ["uchar", "blue"]]
    assert f"element vertex {n}" in head and len(raw) == raw.index(b"end_header\n") + len(b"end_header\n") + 27 * n
    x, c, k = read_ply(with_n, normals=True)
    assert x.tobytes() == xyz.tobytes() and c.tobytes() == rgb.tobytes() and k.dtype == F32 and k.shape == (n, 3) and k.tobytes() == nrm.tobytes()
    assert len(read_ply(with_n)) == 2 and read_ply(with_n)[0].tobytes() == xyz.tobytes()      # the default still returns two values
    with pytest.raises(ValueError, match="normals"):
        write_ply(with_n, xyz, rgb, normals=np.zeros((n + 1, 3), F32))


# ---------------------------------------------------------------- the oracle, by hand
def test_oracle_on_a_plane_worked_by_hand():
    """five points of the plane z = 0 around the query (which is the sixth indexed point): d = (1,0), (-1,0), (0,1), (0,-1), (1,1) and the
    query itself.  S1 = (1, 1, 0), S2 = xx 3, xy 1, yy 3, the z terms 0; c = 6: C = [[3/6 - 1/36, 1/6 - 1/36], [., 3/6 - 1/36]] in x, y and 0
    in z: eigenvalues 0, 1/3, 11/18; normal (0, 0, 1); curvature 0"""
    t = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [1, 1, 0]], F32)
    q = t[:1]
    out = NR.normals(t, q, 8, 2.0)
    assert out["count"].tolist() == [6] and out["valid"].tolist() == [True]
    assert out["mom"][0].tolist() == [1.0, 1.0, 0.0, 3.0, 1.0, 0.0, 3.0, 0.0, 0.0]
    assert out["normal"].tolist() == [[0.0, 0.0, 1.0]] and out["normal"].dtype == F32
    assert out["curvature"].tolist() == [0.0] and out["curvature"].dtype == F32
    assert np.abs(out["lam"][0] - [0.0, 1.0 / 3, 11.0 / 18]).max() < 1e-15
    # the viewpoint: below the plane the normal turns, above it stays; on the plane (s = 0) and not finite: the canonical sign
    for vp, nz in (([0, 0, -5], -1.0), ([3, 3, 5], 1.0), ([7, 7, 0], 1.0), ([0, NAN, -5], 1.0), ([0, 0, -INF], 1.0)):
        assert NR.normals(t, q, 8, 2.0, np.array(vp, F32))["normal"].tolist() == [[0.0, 0.0, nz]], vp
    # a cut-off that leaves the query and its four nearest: S1 = 0, C = diag(2/5, 2/5, 0)
    out = NR.normals(t, q, 8, 1.0)
    assert out["count"].tolist() == [5] and out["mom"][0].tolist() == [0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 2.0, 0.0, 0.0]
    assert out["normal"].tolist() == [[0.0, 0.0, 1.0]] and out["curvature"].tolist() == [0.0]
    # k = 2: fewer than three neighbours
    out = NR.normals(t, q, 2, 2.0)
    assert out["count"].tolist() == [2] and not out["valid"].any() and out["normal"].tolist() == [[0.0, 0.0, 0.0]] and np.isnan(out["curvature"]).all()
    # a tilted plane x + z = 0 with a query beside it: the normal is (1, 0, 1) / sqrt 2 in canonical sign (x leads: the lowest axis on the tie)
    t = np.array([[1, 0, -1], [-1, 0, 1], [0, 1, 0], [0, -1, 0], [2, 2, -2]], F32)
    out = NR.normals(t, np.array([[0.5, 0.25, 3.0]], F32), 5, 10.0)
    assert out["valid"].all() and np.abs(out["n64"][0] - np.array([1, 0, 1]) / np.sqrt(2)).max() < 1e-14 and out["curvature"][0] < 1e-14
    assert NR.canonical(np.array([[-0.6, 0.0, 0.8], [0.6, 0.0, -0.8], [-0.5, 0.5, 0.1]])).tolist() == [[-0.6, 0.0, 0.8], [-0.6, 0.0, 0.8], [0.5, -0.5, -0.1]]


def test_oracle_on_collinear_and_degenerate_neighbourhoods():
    """three collinear points: l1 is 0 (on an axis: exactly) - invalid; a point three times: l2 = 0 - invalid; a query that is not finite;
    an empty target"""
    on_axis = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], F32)
    out = NR.normals(on_axis, on_axis, 3, 5.0)
    assert out["count"].tolist() == [3, 3, 3] and not out["valid"].any() and (out["lam"][:, 1] == 0).all() and (out["lam"][:, 2] > 0).all()
    assert not out["normal"].any() and np.isnan(out["curvature"]).all()
    diagonal = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [5, 5, 5]], F32)
    out = NR.normals(diagonal, diagonal, 4, 20.0)
    assert (out["count"] == 4).all() and not out["valid"].any()
    ratio = out["lam"][:, 1] / out["lam"][:, 2]
    assert (np.abs(ratio) < 0.1 * NR.NORMAL_DEGENERATE).all()      # far below the bar, not near it
    same = np.ones((3, 3), F32)
    out = NR.normals(same, same, 3, 1.0)
    assert (out["count"] == 3).all() and not out["valid"].any() and (out["lam"] == 0).all() and not out["mom"].any()
    q = np.array([[0, NAN, 0], [INF, 0, 0]], F32)
    out = NR.normals(on_axis, q, 3, 5.0)
    assert not out["count"].any() and not out["valid"].any() and not out["mom"].any() and not out["normal"].any() and np.isnan(out["curvature"]).all()
    out = NR.normals(np.zeros((0, 3), F32), on_axis, 3, 5.0)
    assert not out["count"].any() and not out["valid"].any() and not out["mom"].any()


def test_the_test_clouds_meet_the_gpu_tests_preconditions():
    """what tests/test_cloud_normals_gpu.py asserts of the oracle before it compares, checked here too: on the wavy surface at k = 8 and 20 no
    l1 / l2 lies within a factor 10 of the degeneracy bar, no valid row has a gap (l1 - l0) / l2 below 1e-3, the 40 planted floaters have one
    neighbour (themselves), and the oracle's normals are within a degree (median) of the analytic ones at k = 20"""
    pts, planted = R.wavy_surface()
    pairs = R.sorted_neighbours(pts, pts, 20)
    for k in (8, 20):
        out = NR.normals(pts, pts, k, R.FILTER_MAX_DIST, sorted_pairs=pairs)
        lam = out["lam"]
        rows = (out["count"] >= 3) & (lam[:, 2] > 0) & (lam[:, 1] != 0)
        ratio = lam[rows, 1] / lam[rows, 2]
        assert not ((ratio > 0.1 * NR.NORMAL_DEGENERATE) & (ratio < 10 * NR.NORMAL_DEGENERATE)).any()
        assert (out["count"][planted] == 1).all() and not out["valid"][planted].any()
        assert out["valid"].sum() == 4000
        gap = (lam[out["valid"], 1] - lam[out["valid"], 0]) / lam[out["valid"], 2]
        assert gap.min() >= 1e-3
    n = out["n64"][out["valid"]]
    n = n * np.sign(n[:, 2:3])
    cos = np.clip((n * NR.wavy_normal(pts[out["valid"], :2].astype(np.float64))).sum(1), -1, 1)
    assert np.degrees(np.median(np.arccos(cos))) < 1.0
