"""Cloud-to-cloud evaluation (csrc/cloud_eval.hip, cer-mvs_amd/cloud_eval.py), the parts that need no GPU: the C ABI and its argument checks, the
PLY reader against ``fusion.write_ply``, and the arithmetic of the two protocols against a direct numpy restatement."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO

GRID_SYMBOLS = ("cer_grid_partials", "cer_grid_keys_f32", "cer_grid_pack_f32", "cer_grid_cells_count_i64", "cer_grid_cells_i64",
                "cer_grid_nearest_f32")
BIG = 1 << 31


# ---------------------------------------------------------------- C ABI
def test_grid_abi_symbols_are_declared_and_bound():
    from cer_mvs_amd import _lib as L, cloud_eval as CE
    names = L.exported_symbols()
    hdr = open(os.path.join(REPO, "include", "cer_mvs.h")).read()
    for n in GRID_SYMBOLS:
        assert n in names
        assert f" {n}(" in hdr
    for n in GRID_SYMBOLS[1:]:
        assert L._SIGNATURES[n][0] is L._I and L._SIGNATURES[n][1][-1] is L._P      # int f(..., stream)
    assert L.ABI_VERSION >= 1110
    lib = L.load()                                        # (loads without a GPU; refuses a library that lacks a declared symbol)
    assert lib.cer_abi_version() == L.ABI_VERSION
    mk = open(os.path.join(REPO, "cer-mvs_amd", "csrc", "Makefile")).read()
    assert "cloud_eval.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1)
    assert re.search(r"^cloud_eval\.o: CXXFLAGS \+=.*-fno-slp-vectorize", mk, re.M)
    assert f"#define CER_GRID_TILE {CE.GRID_TILE}" in hdr and "#define CER_GRID_COORD_LIMIT (1 << 20)" in hdr and CE.GRID_COORD_LIMIT == 1 << 20
    assert lib.cer_grid_partials(1) == 1 and lib.cer_grid_partials(2048) == 1 and lib.cer_grid_partials(2049) == 2 and lib.cer_grid_partials(0) == 0
    assert lib.cer_grid_partials(-1) == -1 and lib.cer_grid_partials(BIG) == -2


def test_grid_entry_points_refuse_bad_arguments():
    """argument checks run before any launch (the pointers are fake: a launch would fault): negative sizes and null pointers CER_EINVAL, sizes
    of 2^31 and beyond CER_ESHAPE, empty inputs succeed with nothing launched"""
    from cer_mvs_amd import _lib as L
    lib = L.load()
    fake, null = ctypes.c_void_p(4096), None
    o = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    o_nan = (ctypes.c_double * 3)(0.0, float("nan"), 0.0)
    no_o = ctypes.POINTER(ctypes.c_double)()

    keys = lambda n=8, pts=fake, org=o, cell=0.5, clamp=0, out=fake, flag=fake: lib.cer_grid_keys_f32(pts, n, org, cell, clamp, out, flag, null)
    assert keys(n=-1) == -1 and keys(n=BIG) == -2 and keys(n=0) == 0
    assert keys(pts=null) == -1 and keys(out=null) == -1 and keys(flag=null) == -1 and keys(org=no_o) == -1 and keys(org=o_nan) == -1
    assert keys(cell=0.0) == -1 and keys(cell=-1.0) == -1 and keys(cell=float("inf")) == -1 and keys(cell=float("nan")) == -1
    assert keys(n=0, clamp=1, flag=null) == 0

    pack = lambda n=8, pts=fake, order=fake, rec=fake: lib.cer_grid_pack_f32(pts, order, n, rec, null)
    assert pack(n=-1) == -1 and pack(n=BIG) == -2 and pack(n=0) == 0
    assert pack(pts=null) == -1 and pack(order=null) == -1 and pack(rec=null) == -1 and pack(rec=ctypes.c_void_p(4100)) == -3

    count = lambda n=8, k=fake, p=fake, f=fake, t=fake: lib.cer_grid_cells_count_i64(k, n, p, f, t, null)
    assert count(n=-1) == -1 and count(n=BIG) == -2 and count(n=0) == 0
    assert count(k=null) == -1 and count(p=null) == -1 and count(f=null) == -1 and count(t=null) == -1

    cells = lambda n=8, nc=3, k=fake, f=fake, ck=fake, cs=fake: lib.cer_grid_cells_i64(k, n, f, nc, ck, cs, null)
    assert cells(n=-1) == -1 and cells(n=BIG) == -2 and cells(n=0, nc=0) == 0 and cells(nc=0) == 0
    assert cells(nc=-1) == -1 and cells(nc=9) == -2
    assert cells(k=null) == -1 and cells(f=null) == -1 and cells(ck=null) == -1 and cells(cs=null) == -1

    def near(n=8, nc=3, m=5, rec=fake, ck=fake, cs=fake, org=o, cell=0.5, q=fake, qo=null, md=1.0, idx=fake, dist=fake):
        return lib.cer_grid_nearest_f32(rec, n, ck, cs, nc, org, cell, q, qo, m, md, idx, dist, null)
    assert near(n=-1) == -1 and near(m=-1) == -1 and near(nc=-1) == -1
    assert near(n=BIG) == -2 and near(m=BIG) == -2 and near(nc=9) == -2
    assert near(m=0) == 0 and near(n=0, nc=0) == 0 and near(nc=0) == 0
    assert near(rec=null) == -1 and near(ck=null) == -1 and near(cs=null) == -1 and near(q=null) == -1 and near(idx=null) == -1
    assert near(dist=null) == -1 and near(org=no_o) == -1 and near(org=o_nan) == -1 and near(cell=0.0) == -1
    assert near(md=-1.0) == -1 and near(md=float("nan")) == -1
    assert near(md=float("inf")) == -2 and near(md=5000.0, cell=1.0) == -2            # more rings than the search enumerates
    assert near(rec=ctypes.c_void_p(4104)) == -3


def test_python_layer_refuses_cpu_tensors_and_bad_shapes():
    from cer_mvs_amd import cloud_eval as CE
    p = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="CUDA"):
        CE.CloudIndex(p, 0.1)
    with pytest.raises(RuntimeError, match="CUDA"):
        CE.voxel_downsample(p, 0.1)
    with pytest.raises(RuntimeError, match="CUDA"):
        CE.cloud_distances(p, p, 0.1)
    with pytest.raises(RuntimeError, match="CUDA"):
        CE.accuracy_completeness(p, p)
    with pytest.raises(RuntimeError, match="CUDA"):
        CE.fscore(p, p, 0.1)
    assert CE.DEFAULT_CELL_DIVISOR >= 1


# ---------------------------------------------------------------- PLY
def _cloud(n, seed):
    g = np.random.default_rng(seed)
    return g.standard_normal((n, 3)).astype(np.float32), g.integers(0, 256, (n, 3)).astype(np.uint8)


@pytest.mark.parametrize("n", [0, 1, 1000])
def test_write_ply_read_ply_round_trips_bytes(tmp_path, n):
    from cer_mvs_amd import cloud_eval as CE, fusion
    xyz, rgb = _cloud(n, 3)
    if n:
        xyz[0] = [np.nan, -np.inf, -0.0]                 # bytes, not values
    fusion.write_ply(str(tmp_path / "a.ply"), xyz, rgb)
    got_xyz, got_rgb = CE.read_ply(tmp_path / "a.ply")
    assert got_xyz.dtype == np.float32 and got_xyz.shape == (n, 3) and got_rgb.dtype == np.uint8 and got_rgb.shape == (n, 3)
    assert got_xyz.tobytes() == xyz.tobytes() and got_rgb.tobytes() == rgb.tobytes()
    fusion.write_ply(str(tmp_path / "b.ply"), got_xyz, got_rgb)
    assert (tmp_path / "a.ply").read_bytes() == (tmp_path / "b.ply").read_bytes()


def test_read_ply_takes_extra_properties_in_any_order(tmp_path):
    from cer_mvs_amd import cloud_eval as CE
    xyz, rgb = _cloud(257, 5)
    dt = np.dtype([("blue", "u1"), ("z", "<f4"), ("confidence", "<f8"), ("x", "<f4"), ("red", "u1"), ("views", "<u2"), ("y", "<f4"), ("green", "u1")])
    v = np.zeros(len(xyz), dt)
    v["x"], v["y"], v["z"] = xyz.T
    v["red"], v["green"], v["blue"] = rgb.T
    v["confidence"], v["views"] = 0.75, 7
    head = ("ply\nformat binary_little_endian 1.0\ncomment made by a test\nelement vertex 257\nproperty uchar blue\nproperty float z\n"
            "property double confidence\nproperty float x\nproperty uchar red\nproperty ushort views\nproperty float y\nproperty uchar green\n"
            "element face 0\nproperty list uchar int vertex_indices\nend_header\n")
    (tmp_path / "x.ply").write_bytes(head.encode("ascii") + v.tobytes())
    got_xyz, got_rgb = CE.read_ply(tmp_path / "x.ply")
    assert np.array_equal(got_xyz, xyz) and np.array_equal(got_rgb, rgb)
    # no colours: None
    v2 = np.zeros(3, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")]))
    v2["x"] = [1, 2, 3]
    (tmp_path / "y.ply").write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
                                     b"end_header\n" + v2.tobytes())
    got_xyz, got_rgb = CE.read_ply(tmp_path / "y.ply")
    assert got_rgb is None and np.array_equal(got_xyz[:, 0], [1, 2, 3]) and not got_xyz[:, 1:].any()


def test_read_ply_refuses_ascii_and_truncated_files(tmp_path):
    from cer_mvs_amd import cloud_eval as CE
    (tmp_path / "a.ply").write_bytes(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nend_header\n0 0 0\n")
    with pytest.raises(ValueError, match="ascii"):
        CE.read_ply(tmp_path / "a.ply")
    (tmp_path / "b.ply").write_bytes(b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
    with pytest.raises(ValueError, match="binary_big_endian"):
        CE.read_ply(tmp_path / "b.ply")
    (tmp_path / "c.ply").write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n"
                                     b"end_header\n" + bytes(12))
    with pytest.raises(ValueError, match="2 vertices"):
        CE.read_ply(tmp_path / "c.ply")
    (tmp_path / "d.ply").write_bytes(b"not a ply")
    with pytest.raises(ValueError, match="not a PLY"):
        CE.read_ply(tmp_path / "d.ply")


# ---------------------------------------------------------------- the protocols' arithmetic
def metrics_numpy(d_pred, d_gt, max_dist, tau=None):
    """direct restatement: python loops over fp64 values"""
    def mean_below(d):
        vals = [float(v) for v in d if float(v) < max_dist]
        return (sum(vals) / len(vals) if vals else float("nan")), len(vals)
    acc, n_pred_in = mean_below(d_pred)
    comp, n_gt_in = mean_below(d_gt)
    out = {"accuracy": acc, "completeness": comp, "overall": (acc + comp) / 2, "n_pred": len(d_pred), "n_gt": len(d_gt), "n_pred_in": n_pred_in,
           "n_gt_in": n_gt_in}
    if tau is not None:
        p = sum(float(v) < tau for v in d_pred) / len(d_pred) if len(d_pred) else 0.0
        r = sum(float(v) < tau for v in d_gt) / len(d_gt) if len(d_gt) else 0.0
        out.update(precision=p, recall=r, fscore=(2 * p * r / (p + r) if p + r > 0 else 0.0), tau=tau)
    return out


def same_metrics(got, want):
    assert set(got) == set(want)
    for k, w in want.items():
        g = got[k]
        if isinstance(w, int):
            assert g == w, k
        elif np.isnan(w):
            assert np.isnan(g), k
        else:
            assert abs(g - w) <= 1e-12 * abs(w), (k, g, w)


INF = np.inf
CASES = [
    # values at, just below and just above max_dist = 0.5 and tau = 0.25 (both exact in float32)
    ([0.0, 0.25, np.nextafter(np.float32(0.25), np.float32(0)), np.nextafter(np.float32(0.25), np.float32(1)), 0.5,
      np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(1)), 3.0],
     [0.125, 0.5, 0.5, INF, 0.1, 0.2499], 0.5, 0.25),
    ([INF, INF, 0.3], [INF], 0.5, 0.25),                  # one side has nothing inside: nan mean, zero recall
    ([], [0.1, 0.2], 0.5, 0.25),                          # empty inputs
    ([], [], 0.5, 0.25),
    ([0.1, 0.7, 0.2], [0.3], 0.5, None),                  # no tau: the DTU figures alone
    ([0.4, 0.45], [0.3, 0.26], 0.5, 0.25),                # precision = recall = 0: F = 0
]


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_metrics_from_distances_equals_the_restatement(case, kind):
    from cer_mvs_amd import cloud_eval as CE
    a, b, max_dist, tau = CASES[case]
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    want = metrics_numpy(a, b, max_dist, tau)
    got = CE.metrics_from_distances(*((torch.from_numpy(a), torch.from_numpy(b)) if kind == "torch" else (a, b)), max_dist, tau=tau)
    same_metrics(got, want)
    if case == 0:
        assert want["n_pred_in"] == 5 and want["n_gt_in"] == 3 and want["precision"] == 2 / 8     # 0.5 itself is outside, 0.25 itself is not a hit
    if tau is None:
        assert "fscore" not in got


def test_metrics_long_vectors_in_fp64():
    """float32 distances summed in fp64: 1e-12 against the restatement on a vector long enough for a float32 sum to miss that by orders"""
    from cer_mvs_amd import cloud_eval as CE
    g = np.random.default_rng(11)
    a, b = (g.random(200_000) * 0.6).astype(np.float32), (g.random(150_000) * 0.6).astype(np.float32)
    a[::7] = np.inf
    same_metrics(CE.metrics_from_distances(a, b, 0.5, tau=0.1), metrics_numpy(a, b, 0.5, 0.1))
    same_metrics(CE.metrics_from_distances(torch.from_numpy(a), torch.from_numpy(b), 0.5, tau=0.1), metrics_numpy(a, b, 0.5, 0.1))


def test_fscore_is_zero_when_precision_and_recall_are_zero():
    from cer_mvs_amd import cloud_eval as CE
    m = CE.metrics_from_distances(np.array([1.0, 2.0], np.float32), np.array([np.inf], np.float32), 5.0, tau=0.5)
    assert m["precision"] == 0.0 and m["recall"] == 0.0 and m["fscore"] == 0.0
    m = CE.metrics_from_distances(np.array([0.1], np.float32), np.array([0.1, 0.9], np.float32), 5.0, tau=0.5)
    assert m["precision"] == 1.0 and m["recall"] == 0.5 and abs(m["fscore"] - 2 / 3) < 1e-15
