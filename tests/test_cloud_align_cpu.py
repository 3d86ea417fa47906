"""Rigid registration (csrc/cloud_align.hip, cer-mvs_amd/cloud_eval.py rigid_transform / pair_moments / rigid_from_moments / icp / register,
DESIGN.md 3w), the parts that need no GPU: the entry points of ABI 1130 and their argument checks, the Kabsch solve on moments formed by
numpy, the restatement of tests/icp_reference.py against the recovery bar the GPU tests hold the device to, and the argument checks of the
Python layer."""
import ctypes
import os

import numpy as np
import pytest
import torch

import icp_reference as R
from conftest import REPO

ALIGN_SYMBOLS = ("cer_cloud_transform_f32", "cer_cloud_pair_moments_f64")
BIG = 1 << 31
NAN, INF = float("nan"), float("inf")


def test_align_abi_symbols_are_declared_and_bound():
    from cer_mvs_amd import _lib as L
    from cer_mvs_amd import cloud_eval as CE
    names = L.exported_symbols()
    hdr = open(os.path.join(REPO, "include", "cer_mvs.h")).read()
    for n in ALIGN_SYMBOLS:
        assert n in names
        assert f"int {n}(" in hdr
        assert L._SIGNATURES[n][0] is L._I and L._SIGNATURES[n][1][-1] is L._P      # int f(..., stream)
    assert "cer_cloud_moment_partials" in names and "long cer_cloud_moment_partials(long m);" in hdr
    assert L.ABI_VERSION >= 1130
    lib = L.load()                                        # (loads without a GPU; refuses a library that lacks a declared symbol)
    assert lib.cer_abi_version() == L.ABI_VERSION
    assert "ABI 1130" in hdr
    assert f"#define CER_MOMENT_TILE {CE.MOMENT_TILE}\n" in hdr and f"#define CER_MOMENT_COUNT {CE.MOMENT_COUNT}\n" in hdr
    tile = CE.MOMENT_TILE
    for m, want in ((0, 0), (1, 1), (tile, 1), (tile + 1, 2), (1024 * tile + 1, 1025), (BIG - 1, (BIG - 1 + tile - 1) // tile), (-1, -1), (BIG, -2)):
        assert lib.cer_cloud_moment_partials(m) == want


def test_align_entry_points_refuse_bad_arguments():
    """argument checks run before any launch (the pointers are fake: a launch would fault): negative sizes CER_EINVAL, 2^31 and beyond
    CER_ESHAPE, empty inputs succeed with nothing launched, null pointers, an overlapping output and non-finite T / pivot CER_EINVAL"""
    from cer_mvs_amd import _lib as L
    lib = L.load()
    fake, far, null = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 20), None
    eye = (ctypes.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    no_d = ctypes.POINTER(ctypes.c_double)()

    def bad12(i, v):
        t = (ctypes.c_double * 12)(*eye)
        t[i] = v
        return t

    def tr(pts=fake, n=8, T=eye, out=far):
        return lib.cer_cloud_transform_f32(pts, n, T, out, null)
    assert tr(n=-1) == -1 and tr(n=BIG) == -2 and tr(n=BIG + 5) == -2
    assert tr(n=0) == 0 and tr(n=0, pts=null, out=null) == 0
    assert tr(pts=null) == -1 and tr(out=null) == -1 and tr(T=no_d) == -1
    for i in (0, 3, 7, 11):
        for v in (NAN, INF, -INF):
            assert tr(T=bad12(i, v)) == -1
    assert tr(T=bad12(0, NAN), n=0) == -1                                         # (the matrix is looked at before the empty cloud returns)
    assert tr(out=fake) == -1                                                     # in place
    assert tr(out=ctypes.c_void_p(4096 + 12 * 7)) == -1 and tr(pts=ctypes.c_void_p(4096 + 12 * 7), out=fake) == -1      # one row shared
    assert tr(pts=null, out=ctypes.c_void_p(4096 + 12 * 8)) == -1                 # (disjoint: the null pointer is what is refused)

    piv = (ctypes.c_double * 3)(0.0, 0.0, 0.0)

    def mo(a=fake, b=fake, idx=fake, m=8, pivot=piv, part=fake, out=fake):
        return lib.cer_cloud_pair_moments_f64(a, b, idx, m, pivot, part, out, null)
    assert mo(m=-1) == -1 and mo(m=BIG) == -2
    assert mo(m=0) == 0 and mo(m=0, a=null, b=null, idx=null, part=null, out=null) == 0
    assert mo(a=null) == -1 and mo(b=null) == -1 and mo(idx=null) == -1 and mo(part=null) == -1 and mo(out=null) == -1
    assert mo(pivot=no_d) == -1
    for i in range(3):
        for v in (NAN, INF):
            p = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
            p[i] = v
            assert mo(pivot=p) == -1 and mo(pivot=p, m=0) == -1


# ---------------------------------------------------------------- the solve
def numpy_moments(A, B, pivot=(0.0, 0.0, 0.0)):
    """the 17 sums of the pairs (A[i], B[i]) in longdouble, rounded to fp64"""
    A, B = np.asarray(A, np.longdouble) - np.asarray(pivot, np.longdouble), np.asarray(B, np.longdouble) - np.asarray(pivot, np.longdouble)
    D = A - B
    return np.concatenate([[len(A)], A.sum(0), B.sum(0), (A[:, :, None] * B[:, None, :]).sum(0).reshape(-1), [(D * D).sum()]]).astype(np.float64)


def known_pairs(n=500, seed=1, flat=False, offset=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    A = rng.uniform(-10.0, 10.0, (n, 3))
    if flat:
        A[:, 2] = 0.25 * A[:, 0] - 0.5 * A[:, 1] + 1.0       # a plane
    A = A + np.asarray(offset)
    T = R.motion((0.2, -1.0, 0.7), 25.0, (1.5, -2.0, 0.5), centre=A.mean(0))
    return A, R.apply64(T, A), T


def test_rigid_from_moments_recovers_a_known_motion():
    from cer_mvs_amd import cloud_eval as CE
    A, B, T = known_pairs()
    got = CE.rigid_from_moments(numpy_moments(A, B))
    assert got.dtype == np.float64 and got.shape == (4, 4) and np.array_equal(got[3], (0.0, 0.0, 0.0, 1.0))
    assert np.abs(got - T).max() <= 1e-12
    assert np.array_equal(got, R.rigid_from_moments(numpy_moments(A, B)))         # the restatement's solve is the same arithmetic
    assert np.abs(CE.rigid_from_moments(numpy_moments(A, A)) - np.eye(4)).max() <= 1e-12


def test_rigid_from_moments_on_planar_pairs_is_a_proper_rotation():
    """on a plane the third singular value is 0 and a reflection fits as well: the det term picks the rotation"""
    from cer_mvs_amd import cloud_eval as CE
    for seed in range(6):
        A, B, T = known_pairs(seed=seed, flat=True)
        got = CE.rigid_from_moments(numpy_moments(A, B))
        assert abs(np.linalg.det(got[:3, :3]) - 1.0) <= 1e-12
        assert np.abs(got - T).max() <= 1e-10


def test_rigid_from_moments_refuses_what_determines_no_rotation():
    from cer_mvs_amd import cloud_eval as CE
    A, B, _ = known_pairs(n=2)
    with pytest.raises(ValueError, match="3 pairs"):
        CE.rigid_from_moments(numpy_moments(A, B))
    with pytest.raises(ValueError, match="3 pairs"):
        CE.rigid_from_moments(np.zeros(17))
    s = np.linspace(-5.0, 5.0, 50)[:, None]
    line = np.array([1.0, 2.0, 3.0]) + s * np.array([0.5, -1.0, 2.0])
    with pytest.raises(ValueError, match="collinear"):
        CE.rigid_from_moments(numpy_moments(line, line + 0.25))
    same = np.tile([[1.0, 2.0, 3.0]], (5, 1))
    with pytest.raises(ValueError, match="collinear"):
        CE.rigid_from_moments(numpy_moments(same, same))
    with pytest.raises(ValueError, match="17"):
        CE.rigid_from_moments(np.zeros(16))
    with pytest.raises(ValueError, match="pivot"):
        CE.rigid_from_moments(numpy_moments(*known_pairs()[:2]), pivot=(0.0, NAN, 0.0))


def test_rigid_from_moments_with_a_pivot_is_the_same_motion():
    """the pairs sit 270 from the origin: moments about a pivot near them give the motion the plain ones give.  (The plain sums cancel:
    500 products of magnitude 270^2 carry 4e-9 of rounding into a covariance of 1.6e4, 2.5e-13 of rotation, times the lever of 270: 7e-11
    of translation - within the 1e-9 asked for.  Ten times farther out the plain solve itself is off by 1e-8: what the pivot is for.)"""
    from cer_mvs_amd import cloud_eval as CE
    off = (100.0, -200.0, 150.0)
    A, B, T = known_pairs(offset=off)
    plain = CE.rigid_from_moments(numpy_moments(A, B))
    piv = (90.0, -210.0, 140.0)
    pivoted = CE.rigid_from_moments(numpy_moments(A, B, piv), pivot=piv)
    assert np.abs(pivoted - plain).max() <= 1e-9
    assert np.abs(pivoted - T).max() <= 1e-9


# ---------------------------------------------------------------- the restatement
def test_restatement_nearest_keeps_its_contract():
    """the grouped brute force equals the plain one - ties (duplicates: the lowest index), the inclusive cut-off, non-finite points on both sides"""
    rng = np.random.default_rng(5)
    t = rng.uniform(-3.0, 3.0, (700, 3)).astype(np.float32)
    t[100] = t[40]
    t[41] = NAN
    q = rng.uniform(-3.5, 3.5, (500, 3)).astype(np.float32)
    q[0], q[1, 2] = NAN, INF
    q[2] = t[100]
    q[3] = t[7] + np.float32([0.5, 0.0, 0.0])                 # at the cut-off itself along x, whatever else is nearer
    for md in (0.5, 0.05, 10.0):
        a, b = R.nearest(q, t, md), R.nearest_plain(q, t, md)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    d2, idx = R.nearest(q, t, 0.5)
    assert idx[0] == -1 and idx[1] == -1 and idx[2] == 40 and d2[2] == 0.0 and np.isinf(d2[0])
    d2, idx = R.nearest(t[7:8] + np.float32([0.5, 0.0, 0.0]), t[7:8], 0.5)
    dx = np.float64(t[7, 0] + np.float32(0.5)) - np.float64(t[7, 0])
    assert (idx[0] == 0) == (dx * dx <= 0.25)


@pytest.mark.parametrize("name", ["A", "C"])
def test_restatement_meets_the_recovery_bar(name):
    """the bar the device is held to (test_cloud_align_gpu.py): for every point p of the cloud |T p - T_true p| <= 1 float32 ulp of the largest
    |coordinate| of dst.  The only noise of these cases is the half-ulp rounding of dst, which the fit averages: the restatement lands at
    0.002 (A: 6.1e-8) and 0.0006 (C: 3.4e-8) of the bar, after 4 and 12 iterations - inside the default max_iter of 50."""
    src, dst, T_true, max_dist, out = R.reference_run(name)
    assert out["converged"] and out["iterations"] < 50 and out["n_pairs"] == len(src) and out["fitness"] == 1.0
    assert len(out["history"]) == out["iterations"]
    bar = R.ulp32(np.abs(dst).max())
    err = R.recovery_error(out["T"], T_true, src)
    print(f"case {name}: {out['iterations']} iterations, rmse {out['rmse']:.3e}, recovery error {err:.3e} = {err / bar:.4f} of the bar {bar:.3e}")
    assert err <= bar
    if name == "A":                                            # every first match is the right one: the matches of iteration 1 are the planted permutation
        moved = np.abs(R.apply64(T_true, src) - src.astype(np.float64)).max()
        assert moved < 0.2
        first = R.nearest(src, dst, max_dist)[1]
        assert np.abs(dst[first].astype(np.float64) - R.apply64(T_true, src)).max() <= bar


# ---------------------------------------------------------------- the Python layer's argument checks
def good_T():
    return R.motion((0.0, 0.0, 1.0), 10.0, (1.0, 2.0, 3.0))


BAD_T = [np.eye(3), np.zeros((4, 4)), np.eye(4)[None], "identity", [[1, 0, 0, 0]] * 4, np.diag([1.0, 1.0, 1.0, 2.0])]


def test_rigid_transform_refuses_bad_arguments():
    from cer_mvs_amd import cloud_eval as CE
    p = torch.zeros(4, 3)
    for T in BAD_T + [torch.eye(3), torch.zeros(4, 4)]:
        with pytest.raises(ValueError, match="T"):
            CE.rigid_transform(p, T)
    for v in (NAN, INF):
        T = good_T()
        T[1, 2] = v
        with pytest.raises(ValueError, match="finite"):
            CE.rigid_transform(p, T)
    T = good_T()
    T[3, 0] = 1e-30
    with pytest.raises(ValueError, match="last row"):
        CE.rigid_transform(p, T)
    for T in (good_T(), torch.from_numpy(good_T()), good_T().tolist()):           # a good T: the cloud is what is refused
        with pytest.raises(RuntimeError, match="CUDA"):
            CE.rigid_transform(p, T)
    with pytest.raises(RuntimeError, match="CUDA"):
        CE.pair_moments(p, p, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="pivot"):
        CE.pair_moments(p, p, torch.zeros(4, dtype=torch.int64), pivot=(0.0, 1.0))
    with pytest.raises(ValueError, match="pivot"):
        CE.pair_moments(p, p, torch.zeros(4, dtype=torch.int64), pivot=(0.0, 1.0, INF))


def test_icp_and_register_refuse_bad_arguments():
    from cer_mvs_amd import cloud_eval as CE
    p = torch.zeros(4, 3)
    for md in (0.0, -1.0, NAN, INF, 1e-50):                   # (1e-50 is 0 in float32)
        with pytest.raises(ValueError, match="max_dist"):
            CE.icp(p, p, md)
        with pytest.raises(ValueError, match="max_dist"):
            CE.register(p, p, [(None, md, 5)])
    with pytest.raises(ValueError, match="max_iter"):
        CE.icp(p, p, 1.0, max_iter=0)
    with pytest.raises(ValueError, match="tol"):
        CE.icp(p, p, 1.0, tol_fitness=-1.0)
    with pytest.raises(ValueError, match="tol"):
        CE.icp(p, p, 1.0, tol_rmse=NAN)
    for T in BAD_T:
        with pytest.raises(ValueError, match="init"):
            CE.icp(p, p, 1.0, init=T)
        with pytest.raises(ValueError, match="init"):
            CE.register(p, p, [(None, 1.0, 5)], init=T)
    with pytest.raises(RuntimeError, match="CUDA"):
        CE.icp(p, p, 1.0)
    with pytest.raises(RuntimeError, match="CUDA"):
        CE.icp(p, p, 1.0, init=good_T(), max_iter=3)
    for stages in ([], None, 5, [(None, 1.0)], [(1.0, 1.0, 5, 2)], [("coarse", 1.0, 5)]):
        with pytest.raises(ValueError, match="stages"):
            CE.register(p, p, stages)
    with pytest.raises(ValueError, match="stages"):
        CE.register(p, p, [(0.0, 1.0, 5)])                    # a voxel edge must be positive
    with pytest.raises(ValueError, match="max_iter"):
        CE.register(p, p, [(None, 1.0, 0)])
    with pytest.raises(RuntimeError, match="CUDA"):
        CE.register(p, p, [(1.0, 2.0, 5), (None, 1.0, 5)])


def test_align_argument_of_the_protocols_is_checked():
    from cer_mvs_amd import cloud_eval as CE
    p = torch.zeros(4, 3)
    for T in BAD_T:
        with pytest.raises(ValueError, match="T"):
            CE.fscore(p, p, 0.1, align=T)
        with pytest.raises(ValueError, match="T"):
            CE.accuracy_completeness(p, p, align=T)
    with pytest.raises(RuntimeError, match="CUDA"):
        CE.fscore(p, p, 0.1, align=good_T())
    with pytest.raises(RuntimeError, match="CUDA"):
        CE.accuracy_completeness(p, p, align=good_T())
    with pytest.raises(ValueError, match="thin_method"):     # (still the first check)
        CE.accuracy_completeness(p, p, thin_method="matlab", align=np.eye(3))
