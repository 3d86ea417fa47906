"""Point-to-plane ICP (csrc/cloud_align.hip, cer-mvs_amd/cloud_eval.py plane_moments / rigid_from_plane_moments / icp(method="plane"),
DESIGN.md 3z), the parts that need no GPU: the entry points of ABI 1160 and their argument checks in the documented order, the 6x6 solve
against the restatement of tests/icp_plane_reference.py bit for bit, the targets the solve must refuse, the restatement's loop on case C
against point-to-point's iteration count and the recovery bar the GPU tests hold the device to, and the Python layer's argument checks."""
import ctypes
import os

import numpy as np
import pytest
import torch

import icp_plane_reference as P
import icp_reference as R
from conftest import REPO

BIG = 1 << 31
NAN, INF = float("nan"), float("inf")
RECOVERY_ULPS = 0.02                                         # of one float32 ulp of dst's largest |coordinate| (the restatement: 0.00064)


def test_plane_abi_symbols_are_declared_and_bound():
    from cer_mvs_amd import _lib as L
    from cer_mvs_amd import cloud_eval as CE
    names = L.exported_symbols()
    hdr = open(os.path.join(REPO, "include", "cer_mvs.h")).read()
    n = "cer_cloud_plane_moments_f64"
    assert n in names and f"int {n}(" in hdr
    assert L._SIGNATURES[n][0] is L._I and L._SIGNATURES[n][1][-1] is L._P and len(L._SIGNATURES[n][1]) == 9
    assert "cer_cloud_plane_moment_partials" in names and "long cer_cloud_plane_moment_partials(long m);" in hdr
    assert L.ABI_VERSION >= 1160
    lib = L.load()
    assert lib.cer_abi_version() == L.ABI_VERSION
    assert "ABI 1160" in hdr
    assert CE.PLANE_MOMENT_COUNT == P.PLANE_COUNT == 30 and f"#define CER_PLANE_MOMENT_COUNT {CE.PLANE_MOMENT_COUNT}\n" in hdr
    tile = CE.MOMENT_TILE
    for m, want in ((0, 0), (1, 1), (tile, 1), (tile + 1, 2), (1024 * tile + 1, 1025), (BIG - 1, (BIG - 1 + tile - 1) // tile), (-1, -1), (BIG, -2)):
        assert lib.cer_cloud_plane_moment_partials(m) == want == lib.cer_cloud_moment_partials(m)


def test_plane_entry_point_refuses_bad_arguments_in_the_documented_order():
    """every check runs before any launch (the pointers are fake: a launch would fault).  The order: negative size CER_EINVAL (-1); 2^31 and
    beyond CER_ESHAPE (-2); a null or non-finite pivot CER_EINVAL; zero size CER_OK with nothing launched; null pointers CER_EINVAL - each
    case below breaks one rule and every later one, and gets the earlier rule's answer."""
    from cer_mvs_amd import _lib as L
    lib = L.load()
    fake, null = ctypes.c_void_p(4096), None
    piv = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    no_d = ctypes.POINTER(ctypes.c_double)()

    def bad_pivot(i, v):
        p = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
        p[i] = v
        return p

    def mo(a=fake, b=fake, nrm=fake, idx=fake, m=8, pivot=piv, part=fake, out=fake):
        return lib.cer_cloud_plane_moments_f64(a, b, nrm, idx, m, pivot, part, out, null)
    nulls = dict(a=null, b=null, nrm=null, idx=null, part=null, out=null)
    assert mo(m=-1) == -1 and mo(m=-1, pivot=no_d, **nulls) == -1                 # 1: a negative size
    assert mo(m=BIG) == -2 and mo(m=BIG + 7) == -2
    assert mo(m=BIG, pivot=no_d, **nulls) == -2 and mo(m=BIG, pivot=bad_pivot(1, NAN)) == -2      # 2: too large, before the pivot is looked at
    assert mo(pivot=no_d) == -1                                                   # 3: the pivot ...
    for i in range(3):
        for v in (NAN, INF, -INF):
            assert mo(pivot=bad_pivot(i, v)) == -1
            assert mo(pivot=bad_pivot(i, v), m=0) == -1                           # ... before the empty input returns
    assert mo(pivot=no_d, m=0) == -1
    assert mo(m=0) == 0 and mo(m=0, **nulls) == 0                                 # 4: nothing to do, whatever the pointers
    for name in nulls:                                                            # 5: null pointers
        assert mo(**{name: null}) == -1
    assert mo(**nulls) == -1


# ---------------------------------------------------------------- the solve
def explicit_moments(A, B, N, pivot=(0.0, 0.0, 0.0)):
    """the 30 sums of the pairs (A[i], B[i], N[i]) by the restatement, rounded to fp64"""
    return P.plane_moments(A, B, N, np.arange(len(A)), pivot).astype(np.float64)


def wavy_pairs(n=400, seed=2, offset=(0.0, 0.0, 0.0)):
    """points of a wavy surface with its normals, and the same points moved a little: a well-posed step"""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)
    B = np.stack([u, v, 0.3 * np.sin(3 * u) * np.cos(2 * v) + 0.15 * np.sin(7 * v)], 1) * 10.0 + np.asarray(offset)
    N = np.stack([-(0.9 * np.cos(3 * u) * np.cos(2 * v)), -(-0.6 * np.sin(3 * u) * np.sin(2 * v) + 1.05 * np.cos(7 * v)), np.ones(n)], 1)
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    T = R.motion((0.2, -1.0, 0.7), 0.2, (0.01, -0.02, 0.015), centre=B.mean(0))
    A = R.apply64(np.linalg.inv(T), B)
    return A.astype(np.float32), B.astype(np.float32), N.astype(np.float32), T


def test_rigid_from_plane_moments_equals_the_restatement_bit_for_bit():
    from cer_mvs_amd import cloud_eval as CE
    for seed, offset, pivot in ((2, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), (3, (100.0, -200.0, 150.0), (90.0, -210.0, 140.0)), (4, (5.0, 5.0, 5.0), (0.0, 0.0, 0.0))):
        A, B, N, T = wavy_pairs(seed=seed, offset=offset)
        mom = explicit_moments(A, B, N, pivot)
        got, want = CE.rigid_from_plane_moments(mom, pivot), P.rigid_from_plane_moments(mom, pivot)
        assert got.dtype == np.float64 and got.shape == (4, 4) and np.array_equal(got[3], (0.0, 0.0, 0.0, 1.0))
        assert np.array_equal(got.view(np.int64), want.view(np.int64))
        Rm = got[:3, :3]
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-15 and abs(np.linalg.det(Rm) - 1.0) <= 1e-15      # an exact rotation
        before, after = R.recovery_error(np.eye(4), T, A), R.recovery_error(got, T, A)
        print(f"seed {seed}: one step takes the points from {before:.2e} to {after:.2e} of where the planted motion puts them")
        assert after <= 0.02 * before                         # Gauss-Newton from theta = 3.5e-3 rad away: what is left is of relative order theta
        assert P.scaled_spectrum(mom)[0] > 0.01                                   # a well-posed step is far from the rule's 1e-10
    tiny = np.zeros(30)                                                           # the series branch: a step of 1e-12
    tiny[0] = 10.0
    tiny[1:22] = np.eye(6)[P.TRIU]
    tiny[22:28] = 1e-12
    got, want = CE.rigid_from_plane_moments(tiny, (1.0, 2.0, 3.0)), P.rigid_from_plane_moments(tiny, (1.0, 2.0, 3.0))
    assert np.array_equal(got.view(np.int64), want.view(np.int64)) and not np.array_equal(got, np.eye(4))


def degenerate_targets():
    rng = np.random.default_rng(11)
    n = 600
    x, y = rng.uniform(-5.0, 5.0, n), rng.uniform(-5.0, 5.0, n)
    nrm = np.array([0.25, -0.5, 1.0]) / np.linalg.norm([0.25, -0.5, 1.0])
    plane = np.stack([x, y, -0.25 * x + 0.5 * y + 1.0], 1)
    yield "plane", plane, np.tile(nrm, (n, 1))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    yield "sphere", np.array([3.0, -2.0, 7.0]) + 4.0 * d, d
    phi, h = rng.uniform(0.0, 2.0 * np.pi, n), rng.uniform(-6.0, 6.0, n)
    axis, e1, e2 = np.array([1.0, 2.0, 2.0]) / 3.0, np.array([2.0, 1.0, -2.0]) / 3.0, np.array([2.0, -2.0, 1.0]) / 3.0      # an orthonormal frame
    radial = np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2
    yield "cylinder", np.array([1.0, 2.0, 3.0]) + 2.5 * radial + h[:, None] * axis, radial


def test_rigid_from_plane_moments_refuses_what_determines_no_step():
    """fewer than 6 pairs; a plane (its three translations' rows are parallel), a sphere with radial normals (every rotation about the
    centre slides it on itself) and a cylinder (the rotation about and the translation along the axis): the smallest eigenvalue of the
    scaled normal matrix is rounding noise, far below 1e-10"""
    from cer_mvs_amd import cloud_eval as CE
    A, B, N, _ = wavy_pairs()
    for solve in (CE.rigid_from_plane_moments, P.rigid_from_plane_moments):
        with pytest.raises(ValueError, match="6 pairs"):
            solve(explicit_moments(A[:5], B[:5], N[:5]))
        with pytest.raises(ValueError, match="6 pairs"):
            solve(np.zeros(30))
        solve(explicit_moments(A[:6], B[:6], N[:6]))          # six pairs of a curved surface do
    for name, B, N in degenerate_targets():
        A = B + np.array([0.01, -0.02, 0.015])
        mom = explicit_moments(A.astype(np.float32), B.astype(np.float32), N.astype(np.float32))
        low = P.scaled_spectrum(mom)[0]
        print(f"{name}: smallest scaled eigenvalue {low:.2e}")
        assert low <= 1e-10, name
        with pytest.raises(ValueError, match="degenerate"):
            CE.rigid_from_plane_moments(mom)
        with pytest.raises(ValueError, match="degenerate"):
            P.rigid_from_plane_moments(mom)
    flat = np.stack([np.linspace(-1.0, 1.0, 50), np.linspace(-1.0, 1.0, 50) ** 2, np.zeros(50)], 1).astype(np.float32)
    up = np.tile(np.float32([0.0, 0.0, 1.0]), (50, 1))         # normals along z alone: nothing constrains x, y or the rotation about z
    with pytest.raises(ValueError, match="diagonal"):
        CE.rigid_from_plane_moments(explicit_moments(flat + np.float32(0.01), flat, up))
    with pytest.raises(ValueError, match="30"):
        CE.rigid_from_plane_moments(np.zeros(17))
    with pytest.raises(ValueError, match="pivot"):
        CE.rigid_from_plane_moments(explicit_moments(A.astype(np.float32), B.astype(np.float32), N.astype(np.float32)), pivot=(0.0, NAN, 0.0))


# ---------------------------------------------------------------- the restatement
def test_case_c_normals_are_the_surface_normals_of_dst():
    """unit, float32, and orthogonal to the surface: the direction to a point's nearest neighbours in dst has next to no component along it"""
    src, dst, _, _, _ = R.reference_run("C")
    nrm = P.case_c_normals()
    assert nrm.dtype == np.float32 and nrm.shape == dst.shape
    assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1.0).max() <= 2e-7
    some = np.arange(0, len(dst), 97)
    D = dst.astype(np.float64)
    for i in some[:40]:
        d = D - D[i]
        near = np.argsort((d * d).sum(1))[1:7]
        t = d[near] / np.linalg.norm(d[near], axis=1, keepdims=True)
        assert np.abs(t @ nrm[i].astype(np.float64)).max() < 0.2               # (curvature over a neighbour's distance leaves a few degrees)


def test_restatement_plane_loop_beats_point_to_point_and_meets_the_bar():
    """case C with analytic normals: fewer iterations than point-to-point (5 against 12) and the planted motion recovered to <= 0.02 float32
    ulp of the largest coordinate (0.00064: the only noise is dst's half-ulp rounding, which the fit averages)"""
    src, dst, T_true, max_dist, point = R.reference_run("C")
    nrm, out = P.reference_plane_run("analytic")
    assert out["converged"] and out["n_pairs"] == len(src) and out["fitness"] == 1.0 and len(out["history"]) == out["iterations"]
    assert all(len(h) == 3 for h in out["history"])
    assert out["iterations"] < point["iterations"]
    err, bar = R.recovery_error(out["T"], T_true, src), R.ulp32(np.abs(dst).max())
    print(f"plane: {out['iterations']} iterations against {point['iterations']}; plane rmse per iteration {[f'{h[1]:.1e}' for h in out['history']]}; "
          f"recovery error {err:.3e} = {err / bar:.5f} ulp")
    assert err <= RECOVERY_ULPS * bar
    assert out["rmse"] <= out["rmse_point"]                   # |r| = |D . n| <= |D| for unit normals


def test_restatement_with_every_20th_normal_zeroed():
    """a target point without a plane makes no pair: the final matching is the planted bijection, so exactly 19 in 20 src points pair up"""
    src, dst, T_true, max_dist, point = R.reference_run("C")
    nrm, out = P.reference_plane_run("holes")
    assert np.count_nonzero((nrm == 0).all(1)) == len(dst) // 20
    assert out["converged"] and out["fitness"] == 0.95 and out["n_pairs"] == 19 * len(src) // 20
    assert out["iterations"] < point["iterations"]
    assert R.recovery_error(out["T"], T_true, src) <= RECOVERY_ULPS * R.ulp32(np.abs(dst).max())


# ---------------------------------------------------------------- the Python layer's argument checks
def test_method_and_normals_arguments_are_checked():
    from cer_mvs_amd import cloud_eval as CE
    p, n = torch.zeros(4, 3), torch.zeros(4, 3)
    for call in (lambda **kw: CE.icp(p, p, 1.0, **kw), lambda **kw: CE.register(p, p, [(None, 1.0, 5)], **kw)):
        with pytest.raises(ValueError, match="method"):
            call(method="point", dst_normals=n)
        with pytest.raises(ValueError, match="method"):
            call(dst_normals=n)                               # (the default is "point")
        with pytest.raises(ValueError, match="method"):
            call(method="point", normals={"k": 20})
        with pytest.raises(ValueError, match="method"):
            call(method="symmetric")
        with pytest.raises(ValueError, match="method"):
            call(method=None)
        with pytest.raises(RuntimeError, match="CUDA"):       # a good method: the clouds are what is refused
            call(method="plane", dst_normals=n)
        with pytest.raises(RuntimeError, match="CUDA"):
            call(method="plane")
    with pytest.raises(ValueError, match="max_dist"):
        CE.icp(p, p, 0.0, method="plane")
    with pytest.raises(RuntimeError, match="CUDA"):
        CE.plane_moments(p, p, n, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="pivot"):
        CE.plane_moments(p, p, n, torch.zeros(4, dtype=torch.int64), pivot=(0.0, INF, 1.0))
