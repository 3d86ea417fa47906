"""k nearest neighbours, the count within a radius and the outlier filters (csrc/cloud_eval.hip grid_knn_kernel / grid_count_within_kernel,
cer-mvs_amd/cloud_eval.py CloudIndex.knn / knn_mean_distance / count_within, remove_statistical_outliers / remove_radius_outliers),
the parts that need no GPU: the entry points of ABI 1140 and their argument checks in the documented order, the ValueErrors of the Python
layer, and the oracle of tests/knn_reference.py against a case worked by hand."""
import ctypes
import os

import numpy as np
import pytest
import torch

import knn_reference as R
from conftest import REPO

KNN_SYMBOLS = ("cer_grid_knn_f32", "cer_grid_count_within_f32")
BIG = 1 << 31
NAN, INF = float("nan"), float("inf")


def test_knn_abi_symbols_are_declared_and_bound():
    from cer_mvs_amd import _lib as L
    from cer_mvs_amd import cloud_eval as CE
    names = L.exported_symbols()
    hdr = open(os.path.join(REPO, "include", "cer_mvs.h")).read()
    for n in KNN_SYMBOLS:
        assert n in names
        assert f"int {n}(const void* records, long n, const long long* cell_keys, const long long* cell_start, long ncells" in hdr
        assert L._SIGNATURES[n][0] is L._I and L._SIGNATURES[n][1][-1] is L._P      # int f(..., stream)
        assert L._SIGNATURES[n][1][:7] == L._SIGNATURES["cer_grid_nearest_f32"][1][:7]      # CloudIndex.grid_args()
    assert len(L._SIGNATURES["cer_grid_knn_f32"][1]) == 17 and len(L._SIGNATURES["cer_grid_count_within_f32"][1]) == 13
    assert L.ABI_VERSION >= 1140
    lib = L.load()                                        # (loads without a GPU; refuses a library that lacks a declared symbol)
    assert lib.cer_abi_version() == L.ABI_VERSION
    assert "ABI 1140" in hdr
    assert f"#define CER_KNN_MAX {CE.KNN_MAX}\n" in hdr and CE.KNN_MAX == 32 == R.KNN_MAX
    for word in ("long long* idx, float* dist,", "int* count, double* mean, void* stream);", "float radius,", "int* count, void* stream);"):
        assert word in hdr


def test_knn_entry_points_refuse_bad_arguments_in_the_documented_order():
    """argument checks run before any launch (the pointers are fake: a launch would fault).  The order is grid_search_rings': sizes; frame,
    reach and k < 1 -> CER_EINVAL; ncells > n and k > CER_KNN_MAX -> CER_ESHAPE; rings -> CER_ESHAPE; an empty side -> CER_OK; null pointers
    (count among them; idx, dist and mean may be null) -> CER_EINVAL; alignment -> CER_EALIGN.  Two faults at once: the earlier check answers."""
    from cer_mvs_amd import _lib as L
    lib = L.load()
    fake, null = ctypes.c_void_p(4096), None
    o = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    o_nan = (ctypes.c_double * 3)(0.0, NAN, 0.0)
    no_o = ctypes.POINTER(ctypes.c_double)()
    odd = ctypes.c_void_p(4104)

    def knn(n=8, nc=3, m=5, rec=fake, ck=fake, cs=fake, org=o, cell=0.5, q=fake, qo=null, k=4, md=1.0, idx=fake, dist=fake, count=fake, mean=fake):
        return lib.cer_grid_knn_f32(rec, n, ck, cs, nc, org, cell, q, qo, m, k, md, idx, dist, count, mean, null)
    assert knn(n=-1) == -1 and knn(m=-1) == -1 and knn(nc=-1) == -1
    assert knn(n=BIG) == -2 and knn(m=BIG) == -2 and knn(nc=9) == -2
    assert knn(org=no_o) == -1 and knn(org=o_nan) == -1 and knn(cell=0.0) == -1 and knn(cell=NAN) == -1
    assert knn(md=-1.0) == -1 and knn(md=NAN) == -1
    assert knn(k=0) == -1 and knn(k=-3) == -1
    assert knn(k=33) == -2 and knn(k=1 << 20) == -2
    for k in (1, 8, 9, 16, 17, 32):                       # every width: the checks pass and an empty side launches nothing
        assert knn(k=k, m=0) == 0
    assert knn(md=INF) == -2 and knn(md=5000.0, cell=1.0) == -2            # more rings than the search enumerates
    assert knn(m=0) == 0 and knn(n=0, nc=0) == 0 and knn(nc=0) == 0
    assert knn(m=0, rec=null, ck=null, cs=null, q=null, idx=null, dist=null, count=null, mean=null) == 0
    assert knn(rec=null) == -1 and knn(ck=null) == -1 and knn(cs=null) == -1 and knn(q=null) == -1
    assert knn(count=null) == -1 and knn(count=null, idx=null, dist=null, mean=null) == -1
    assert knn(rec=odd) == -3
    # the order: sizes before k, k < 1 (CER_EINVAL) before k > 32's class (CER_ESHAPE: nc > n), both before the empty side and the pointers
    assert knn(n=BIG, k=0) == -2 and knn(m=-1, k=33) == -1
    assert knn(k=0, nc=9) == -1 and knn(k=0, md=INF) == -1 and knn(k=0, m=0) == -1 and knn(k=0, count=null) == -1
    assert knn(k=33, md=-1.0) == -1 and knn(k=33, m=0) == -2 and knn(k=33, count=null) == -2 and knn(k=33, rec=odd) == -2
    assert knn(md=INF, m=0) == -2 and knn(md=INF, count=null) == -2
    assert knn(count=null, rec=odd) == -1

    def cnt(n=8, nc=3, m=5, rec=fake, ck=fake, cs=fake, org=o, cell=0.5, q=fake, qo=null, r=1.0, count=fake):
        return lib.cer_grid_count_within_f32(rec, n, ck, cs, nc, org, cell, q, qo, m, r, count, null)
    assert cnt(n=-1) == -1 and cnt(m=-1) == -1 and cnt(nc=-1) == -1
    assert cnt(n=BIG) == -2 and cnt(m=BIG) == -2 and cnt(nc=9) == -2
    assert cnt(org=no_o) == -1 and cnt(org=o_nan) == -1 and cnt(cell=0.0) == -1 and cnt(cell=INF) == -1
    assert cnt(r=-1.0) == -1 and cnt(r=NAN) == -1
    assert cnt(r=INF) == -2 and cnt(r=5000.0, cell=1.0) == -2
    assert cnt(r=0.0, m=0) == 0 and cnt(m=0) == 0 and cnt(n=0, nc=0) == 0 and cnt(nc=0) == 0
    assert cnt(m=0, rec=null, ck=null, cs=null, q=null, count=null) == 0
    assert cnt(rec=null) == -1 and cnt(ck=null) == -1 and cnt(cs=null) == -1 and cnt(q=null) == -1 and cnt(count=null) == -1
    assert cnt(rec=odd) == -3
    assert cnt(r=-1.0, nc=9) == -1 and cnt(r=INF, m=0) == -2 and cnt(count=null, rec=odd) == -1


def test_python_layer_raises_value_errors():
    """``k`` outside 1 .. 32 and bad distances are refused before the tensors are looked at; a tensor that is not on the device is not a
    ValueError but the package's "no CPU fallback\""""
    from cer_mvs_amd import cloud_eval as CE
    index = CE.CloudIndex.__new__(CE.CloudIndex)          # (no GPU here: the checks below come before the index is touched)
    p = torch.zeros(4, 3)
    for k in (0, -1, 33, 100):
        with pytest.raises(ValueError, match="1 .. 32"):
            index.knn(p, k, 0.1)
        with pytest.raises(ValueError, match="1 .. 32"):
            index.knn_mean_distance(p, k, 0.1)
        with pytest.raises(ValueError, match="1 .. 32"):
            CE.remove_statistical_outliers(p, k=k)
    for bad in (-1.0, NAN):
        with pytest.raises(ValueError, match="max_dist"):
            index.knn(p, 4, bad)
        with pytest.raises(ValueError, match="max_dist"):
            CE.remove_statistical_outliers(p, max_dist=bad)
        with pytest.raises(ValueError, match="radius"):
            index.count_within(p, bad)
        with pytest.raises(ValueError, match="radius"):
            CE.remove_radius_outliers(p, bad, 3)
    with pytest.raises(ValueError, match="std_ratio"):
        CE.remove_statistical_outliers(p, std_ratio=NAN)
    with pytest.raises(ValueError, match="cell"):
        CE.remove_statistical_outliers(p, cell=0.0)
    with pytest.raises(ValueError, match="cell"):
        CE.remove_radius_outliers(p, 0.1, 3, cell=-1.0)
    with pytest.raises(ValueError, match="min_neighbours"):
        CE.remove_radius_outliers(p, 0.1, -1)
    for clean in ("radius", {}, {"method": "median"}, {"method": "radius", "radius": 0.1}, {"method": "radius", "radius": 0.1, "min_neighbours": 2, "k": 3},
                  {"method": "statistical", "radius": 0.1}):
        with pytest.raises(ValueError, match="clean"):
            CE.clean_cloud(p, clean)
    with pytest.raises(RuntimeError, match="CUDA"):
        index.knn(p, 4, 0.1)
    with pytest.raises(RuntimeError, match="CUDA"):
        index.count_within(p, 0.1)
    with pytest.raises(RuntimeError, match="CUDA"):
        CE.remove_statistical_outliers(p)
    with pytest.raises(RuntimeError, match="CUDA"):
        CE.remove_radius_outliers(p, 0.1, 3)


def test_reconstruct_scan_takes_clean_and_defaults_to_none():
    import inspect
    from cer_mvs_amd.scan import reconstruct_scan
    par = inspect.signature(reconstruct_scan).parameters
    assert "clean" in par and par["clean"].default is None
    assert "masks" in reconstruct_scan.__doc__ and "stay as fused" in reconstruct_scan.__doc__


# ---------------------------------------------------------------- the oracle, by hand
def test_oracle_on_five_points_worked_by_hand():
    """targets on the x axis at 0, 1, 1 (a duplicate), 3 and one that is not finite; the query sits on target 0"""
    t = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [3, 0, 0], [NAN, 0, 0]], np.float32)
    q = np.array([[0, 0, 0], [2, 0, 0], [0, INF, 0], [50, 0, 0]], np.float32)
    dist, idx, count, mean = R.knn(t, q, 3, 2.0)
    assert idx.tolist() == [[0, 1, 2], [1, 2, 3], [-1, -1, -1], [-1, -1, -1]]      # the duplicate: the lower index first; 3 is 1 from the query at 2
    assert dist.tolist() == [[0.0, 1.0, 1.0], [1.0, 1.0, 1.0], [INF, INF, INF], [INF, INF, INF]] and dist.dtype == np.float32
    assert count.tolist() == [3, 3, 0, 0] and count.dtype == np.int32
    assert mean.tolist() == [(0.0 + 1.0 + 1.0) / 3, 1.0, INF, INF]
    dist, idx, count, mean = R.knn(t, q, 4, 3.0)          # the cut-off is inclusive: the point at 3 is the query's fourth
    assert idx[0].tolist() == [0, 1, 2, 3] and dist[0].tolist() == [0.0, 1.0, 1.0, 3.0] and count[0] == 4 and mean[0] == 5.0 / 4
    assert idx[1].tolist() == [1, 2, 3, 0] and dist[1].tolist() == [1.0, 1.0, 1.0, 2.0]      # three at distance 1: ascending indices
    dist, idx, count, mean = R.knn(t, q, 4, 2.5)          # a partly filled row
    assert idx[0].tolist() == [0, 1, 2, -1] and dist[0].tolist() == [0.0, 1.0, 1.0, INF] and count[0] == 3 and mean[0] == 2.0 / 3
    dist, idx, count, mean = R.knn(t, q, 8, 100.0)        # fewer targets than k: the non-finite one never counts
    assert count.tolist() == [4, 4, 0, 4] and idx[3].tolist() == [3, 1, 2, 0, -1, -1, -1, -1]
    assert mean[3] == (((47.0 + 49.0) + 49.0) + 50.0) / 4
    dist1, idx1, count1, _ = R.knn(t, q, 1, 0.0)          # max_dist 0: a coincident point alone
    assert idx1[:, 0].tolist() == [0, -1, -1, -1] and count1.tolist() == [1, 0, 0, 0]
    assert R.count_within(t, q, 1.0).tolist() == [3, 3, 0, 0] and R.count_within(t, q, 0.0).tolist() == [1, 0, 0, 0]
    assert R.count_within(t, q, 0.99).tolist() == [1, 0, 0, 0] and R.count_within(t, q, 47.0).tolist() == [4, 4, 0, 1]
    assert R.count_within(t, q, 1.0).dtype == np.int32 and R.count_within(np.zeros((0, 3)), q, 1.0).tolist() == [0, 0, 0, 0]
    # the filters: of the four finite targets every one has two neighbours within 1 (itself included) but the point at 3
    keep, info = R.statistical_outliers(t, 2, 1.0, 1.0)
    assert info["valid"].tolist() == [True, True, True, False, False] and info["n_valid"] == 3
    assert info["mean"][:3].tolist() == [0.5, 0.0, 0.0] and info["mu"] == 0.5 / 3
    assert abs(info["sigma"] - np.sqrt(((0.5 - 0.5 / 3) ** 2 + 2 * (0.5 / 3) ** 2) / 2)) < 1e-15
    assert keep.tolist() == [1, 2]                        # 0.5 is above mu + sigma = 0.455..
    assert R.statistical_outliers(t, 2, 2.0, 1.0)[0].tolist() == [0, 1, 2]
    assert R.statistical_outliers(t[3:], 1, 1.0, 1.0)[0].tolist() == [0]      # one valid point: kept
    assert R.radius_outliers(t, 1.0, 2).tolist() == [0, 1, 2] and R.radius_outliers(t, 1.0, 3).tolist() == []
    assert R.radius_outliers(t, 2.0, 3).tolist() == [1, 2]


def test_the_filter_cloud_meets_its_preconditions():
    """the wavy surface of the GPU test: the planted points are isolated at max_dist, both filters keep and drop surface points, and no mean
    lies within 1e-9 (relative) of a threshold - what makes the kept SETS comparable index for index"""
    pts, planted = R.wavy_surface()
    assert len(pts) == 4040 and len(planted) == 40
    pairs = R.sorted_neighbours(pts, pts, 20)
    assert (R.count_within(pts, pts[planted], R.FILTER_MAX_DIST) == 1).all()
    surface = np.setdiff1d(np.arange(len(pts)), planted)
    for k in (8, 20):
        keep, info = R.statistical_outliers(pts, k, 2.0, R.FILTER_MAX_DIST, (pairs[0][:, :k], pairs[1][:, :k]))
        assert not np.isin(planted, keep).any() and not info["valid"][planted].any()
        assert 0 < np.isin(surface, keep).sum() < len(surface)
        assert (info["valid"][surface] & ~np.isin(surface, keep)).any()      # a surface point with k neighbours, above the threshold
        thr = info["threshold"]
        assert np.abs(info["mean"][info["valid"]] - thr).min() > 1e-9 * thr
    keep = R.radius_outliers(pts, R.FILTER_RADIUS, R.FILTER_MIN_NEIGHBOURS)
    assert not np.isin(planted, keep).any() and 0 < len(keep) < len(surface)
