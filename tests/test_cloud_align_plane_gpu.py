"""Point-to-plane ICP on the MI355X (csrc/cloud_align.hip, cer-mvs_amd/cloud_eval.py) against the numpy restatement of
tests/icp_plane_reference.py.

The moments.  With coordinates that are integers in [-64, 64], normals that are integers in [-2, 2] and an integer pivot every term and every
partial sum is an integer below 2^53, so whatever the summation order all 30 sums are exact and must equal int64 numpy sums bit for bit -
any indexing error shows without a tolerance.  With float data sum k must lie within c_k * 2^-53 * sum|term| of the longdouble reference,
c_k counted from the kernel's own arithmetic and tree (u = 2^-53; first order, as test_cloud_align_gpu.py does for the 17 sums):
    roundings of a term   1: 0.  A = a - pivot: 1; n: 0 (a promoted float32).  c_i = A_j n_k - A_k n_j: each product carries A's rounding and
                          its own, the subtraction 1: 3.  D = a - b: 1; r = (Dx nx + Dy ny) + Dz nz: D 1, a product 1, two additions 2: 4.  A
                          product of two such quantities carries both counts and its own rounding: J_i J_j = 7 (c c), 4 (c n), 1 (n n);
                          J_i r = 8 (c r), 5 (n r); r r = 9; d2 = 5 (as in 3w).  (c and r are differences: their roundings are relative to
                          the products inside, which can exceed |c| and |r| themselves.  The bound below takes sum|term| as it is - it asks
                          for more than this count proves when many pairs cancel at once; on these inputs they do not.)
    pass 1                a thread's 8 terms in sequence 8; the butterfly over 64 lanes 6; four waves as (w0 + w1) + (w2 + w3) 2
    pass 2                ceil(P / 1024) partials per thread in sequence, P = ceil(m / 2048); butterfly 6; sixteen waves pairwise 4
so c_k = term_k + 8 + 6 + 2 + ceil(P / 1024) + 6 + 4.

The loop: case C of icp_reference.py with the analytic normals of icp_plane_reference.case_c_normals().  Measured maxima go to
profiles/cloud_align_plane_parity.json under CER_PARITY_RECORD=1 (a run of the whole module); a plain run writes nothing.  Measured on an
MI355X: moments, largest |err| / bound 0.044; one iteration on case C, rotation 7.8e-17 against a bound of 5.9e-14, translation 2.1e-14
against 3.2e-11 (scaled condition number 33); the loop 5 iterations against point-to-point's 12, the planted motion to 3.9e-8 (0.00064 ulp;
bar 0.02), the restatement's T to 1.1e-15 of the extent; estimated normals 5 iterations, 0.0019 ulp; register 6 + 5 iterations, 0.00044 ulp."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import icp_plane_reference as P
import icp_reference as R
from conftest import REPO

pytestmark = pytest.mark.gpu

F32 = np.float32
U = 2.0 ** -53
RECOVERY_ULPS = 0.02                                         # of one float32 ulp of dst's largest |coordinate|
_RJ = np.array([3, 3, 3, 0, 0, 0])                           # roundings of J = (c, n); r: 4
TERM_ROUNDINGS = np.array([0] + [_RJ[i] + _RJ[j] + 1 for i, j in zip(*P.TRIU)] + [rj + 4 + 1 for rj in _RJ] + [4 + 4 + 1, 5], np.float64)
RECORD = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _record(dev):
    yield
    target = os.environ.get("CER_PARITY_RECORD", "")
    if target:
        path = os.path.join(REPO, "profiles", "cloud_align_plane_parity.json") if target == "1" else target
        with open(path, "w") as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
            f.write("\n")


def on(dev, array):
    """a tensor on the device with a copy of ``array`` (the shared cases are read-only)"""
    return torch.from_numpy(np.array(array)).to(dev)


def extent(points):
    return float((points.max(0).astype(np.float64) - points.min(0).astype(np.float64)).max())


# ---------------------------------------------------------------- moments
INTEGER_SIZES = [1, 255, 256, 257, 2049, 2097153]            # the last: 1025 partials, one more than the second pass's block is wide
FLOAT_SIZES = [257, 2049]


def plane_case(m, integer, seed):
    """a, b, nrm, idx, pivot: a random map into 1000 target points with about one in eight -1, a few non-finite rows of a, and normals
    with zero rows (and, for float data, a non-finite one) among them"""
    rng = np.random.default_rng(seed)
    nb = 1000
    if integer:
        a, b = rng.integers(-64, 65, (m, 3)).astype(F32), rng.integers(-64, 65, (nb, 3)).astype(F32)
        nrm = rng.integers(-2, 3, (nb, 3)).astype(F32)
        pivot = (-7.0, 11.0, 3.0)
    else:
        a = (rng.uniform(-40.0, 40.0, (m, 3)) + np.array([10.0, 20.0, 500.0])).astype(F32)
        b = (rng.uniform(-40.0, 40.0, (nb, 3)) + np.array([10.0, 20.0, 500.0])).astype(F32)
        nrm = rng.normal(size=(nb, 3))
        nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F32)
        nrm[5], nrm[17, 1] = np.nan, np.inf
        pivot = (-30.0, -20.0, 460.0)
    nrm[::16] = 0.0                                           # "no plane"
    idx = rng.integers(0, nb, m)
    idx[rng.uniform(size=m) < 0.125] = -1
    if m == 1:
        idx[0] = 1                                            # (the single pair is a pair)
        nrm[1] = (1.0, -2.0, 2.0) if integer else (0.6, 0.0, 0.8)
    for j, v in zip(rng.integers(0, m, min(m // 50, 7)), (np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan, np.nan)):
        a[j, rng.integers(0, 3)] = v
    return a, b, nrm, idx.astype(np.int64), pivot


def device_plane_moments(dev, a, b, nrm, idx, pivot):
    from cer_mvs_amd import cloud_eval as CE
    return CE.plane_moments(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), torch.from_numpy(nrm).to(dev), torch.from_numpy(idx).to(dev),
                            pivot)


def int64_plane_moments(a, b, nrm, idx, pivot):
    """the 30 sums of integer data in int64 - no rounding anywhere"""
    sel = P.plane_pairs(a, nrm, idx)
    q = idx[sel]
    pa, pb, n = a[sel].astype(np.int64), b[q].astype(np.int64), nrm[q].astype(np.int64)
    A, D = pa - np.asarray(pivot, np.int64), pa - pb
    r = D[:, 0] * n[:, 0] + D[:, 1] * n[:, 1] + D[:, 2] * n[:, 2]
    J = [A[:, 1] * n[:, 2] - A[:, 2] * n[:, 1], A[:, 2] * n[:, 0] - A[:, 0] * n[:, 2], A[:, 0] * n[:, 1] - A[:, 1] * n[:, 0], n[:, 0], n[:, 1], n[:, 2]]
    cols = [np.ones(len(A), np.int64)] + [J[i] * J[j] for i, j in zip(*P.TRIU)] + [J[i] * r for i in range(6)] + [r * r, (D * D).sum(1)]
    return np.array([int(c.sum()) for c in cols], np.int64), max(int(np.abs(c).sum()) for c in cols)


def plane_constants(m):
    from cer_mvs_amd import _lib as L
    from cer_mvs_amd import cloud_eval as CE
    Pn = int(L.load().cer_cloud_plane_moment_partials(m))
    assert Pn == -(-m // CE.MOMENT_TILE)
    return TERM_ROUNDINGS + (CE.MOMENT_TILE // 256 + 6 + 2) + (-(-Pn // 1024) + 6 + 4), Pn


@pytest.mark.parametrize("m", INTEGER_SIZES)
def test_plane_moments_of_integer_data_are_exact(dev, m):
    a, b, nrm, idx, pivot = plane_case(m, True, seed=m)
    want, largest = int64_plane_moments(a, b, nrm, idx, pivot)
    assert largest < 2 ** 53                                  # every partial sum, in any order, is an exact fp64 integer
    got = device_plane_moments(dev, a, b, nrm, idx, pivot)
    assert got.dtype == np.float64 and got.shape == (30,)
    assert got[0] == np.count_nonzero(P.plane_pairs(a, nrm, idx)) and (m == 1 or got[0] < np.count_nonzero(idx >= 0))      # zero normals drop pairs
    assert np.array_equal(got, want.astype(np.float64)), (got - want.astype(np.float64))
    assert np.array_equal(got.view(np.int64), want.astype(np.float64).view(np.int64))
    if m <= 2049:                                             # the two references agree (the longdouble one is what the float test uses)
        assert np.array_equal(P.plane_moments(a, b, nrm, idx, pivot).astype(np.float64), want.astype(np.float64))
    assert np.array_equal(got.view(np.int64), device_plane_moments(dev, a, b, nrm, idx, pivot).view(np.int64))      # two launches: the same bits


@pytest.mark.parametrize("m", FLOAT_SIZES)
def test_plane_moments_of_float_data_are_within_the_counted_bound(dev, m):
    a, b, nrm, idx, pivot = plane_case(m, False, seed=m + 1)
    want, mag = P.plane_moments(a, b, nrm, idx, pivot, with_magnitude=True)
    c, Pn = plane_constants(m)
    got = device_plane_moments(dev, a, b, nrm, idx, pivot)
    assert got[0] == float(want[0]) > 0                       # k is exact
    err = np.abs(got.astype(np.longdouble) - want)
    bound = c.astype(np.longdouble) * U * mag
    ratio = float((err[1:] / bound[1:]).max())
    print(f"m = {m}: {Pn} partials, k = {int(got[0])}, max |err| / bound = {ratio:.3f}")
    RECORD.setdefault("moments_max_err_over_bound", {})[str(m)] = ratio
    assert (err <= bound).all(), (err / np.maximum(bound, np.longdouble(1e-300))).astype(np.float64)
    again = device_plane_moments(dev, a, b, nrm, idx, pivot)
    assert np.array_equal(got.view(np.int64), again.view(np.int64))                                   # determinism
    plain = device_plane_moments(dev, a, b, nrm, idx, None)   # the default pivot is the origin
    assert np.array_equal(plain.view(np.int64), device_plane_moments(dev, a, b, nrm, idx, (0.0, 0.0, 0.0)).view(np.int64))
    assert np.array_equal(plain[[0, 28, 29]], got[[0, 28, 29]])                                       # k, sum r^2 and sum d2 do not see the pivot
    scaled = device_plane_moments(dev, a, b, (2.0 * nrm).astype(F32), idx, pivot)                      # normals are used as given: 2 n, exactly
    assert np.array_equal(scaled[28], 4.0 * got[28]) and np.array_equal(scaled[29], got[29]) and np.array_equal(scaled[22:28], 4.0 * got[22:28])


def test_plane_moments_without_pairs_are_zero(dev):
    from cer_mvs_amd import cloud_eval as CE
    a, b, nrm, idx, pivot = plane_case(3000, False, seed=9)
    zeros = np.zeros(30)
    got = device_plane_moments(dev, a, b, nrm, np.full_like(idx, -1), pivot)                          # no match at all
    assert np.array_equal(got, zeros) and not np.signbit(got).any()
    got = device_plane_moments(dev, a, b, np.zeros_like(nrm), np.abs(idx), pivot)                     # no target has a plane
    assert np.array_equal(got, zeros) and not np.signbit(got).any()
    assert np.array_equal(device_plane_moments(dev, a, b, np.full_like(nrm, np.nan), np.abs(idx), pivot), zeros)
    a[:] = np.nan                                             # every a non-finite: no pair either
    assert np.array_equal(device_plane_moments(dev, a, b, nrm, np.abs(idx), pivot), zeros)
    p, n = torch.from_numpy(b).to(dev), torch.from_numpy(nrm).to(dev)
    e = torch.empty(0, 3, device=dev)                         # m = 0: nothing is launched
    assert np.array_equal(CE.plane_moments(e, p, n, torch.empty(0, dtype=torch.int64, device=dev)), zeros)
    for bad in (torch.full((1000,), 1000, dtype=torch.int64), torch.full((1000,), -2, dtype=torch.int64), torch.zeros(999, dtype=torch.int64),
                torch.zeros(1000, dtype=torch.int32)):
        with pytest.raises(ValueError, match="idx"):
            CE.plane_moments(p, p, n, bad.to(dev))
    ok = torch.zeros(1000, dtype=torch.int64, device=dev)
    for bad in (n[:999], n[:, :2], n.reshape(-1)):
        with pytest.raises(ValueError, match="normals"):
            CE.plane_moments(p, p, bad, ok)
    with pytest.raises(RuntimeError, match="normals"):
        CE.plane_moments(p, p, n.double(), ok)
    with pytest.raises(RuntimeError, match="normals"):
        CE.plane_moments(p, p, n.cpu(), ok)


# ---------------------------------------------------------------- one iteration
def test_one_plane_iteration_on_case_c(dev):
    """at T = I: the matches and k are the restatement's, and the solved step is within the moments' bound propagated through the solve.
    With e = c u sum|term| the moments' bounds, E the symmetric 6x6 of e[1:22] and f = e[22:28]: M x = -g moves, to first order, by
      |dx| <= |M^-1| (f + E |x|) + 2 * 100 u |M^-1| |M| |x|    entry by entry
    - the second term the backward error of LAPACK's 6x6 solve on either side, taken as 100 u (ten times the textbook constant, as 3w
    does); the diagonal scaling is positive and diagonal, so it leaves the entrywise bound as it is.  Its size is the condition number's:
    cond(Ms) is printed.  R = exp([w]x) moves by ||dR||_F <= sqrt 2 |dw| + 16 u and the translation pivot - R pivot + t by |dt| + ||dR||_F
    |pivot| + 16 u (|pivot| + |t|)."""
    from cer_mvs_amd import cloud_eval as CE
    src, dst, T_true, max_dist, _ = R.reference_run("C")
    nrm, ref_run = P.reference_plane_run("analytic")
    s, d, n = on(dev, src), on(dev, dst), on(dev, nrm)
    index = CE.CloudIndex(d, max_dist / CE.DEFAULT_CELL_DIVISOR)
    idx = index.nearest(s, max_dist)[1]
    idx_ref = R.nearest(src, dst, max_dist)[1]
    assert np.array_equal(idx.cpu().numpy(), idx_ref)
    pivot = np.array([float(v) for v in index.origin])
    assert np.array_equal(pivot, dst.min(0).astype(np.float64))
    got = CE.plane_moments(s, d, n, idx, pivot)
    want, mag = P.plane_moments(src, dst, nrm, idx_ref, pivot, with_magnitude=True)
    c, _ = plane_constants(len(src))
    assert (np.abs(got.astype(np.longdouble) - want) <= c.astype(np.longdouble) * U * mag).all()
    e = c * U * mag.astype(np.float64)
    k = int(got[0])
    assert k == int(want[0]) == np.count_nonzero(idx_ref >= 0) and k / len(src) == ref_run["history"][0][0]
    w = want.astype(np.float64)
    assert ref_run["history"][0][1] == math.sqrt(w[28] / k) and ref_run["history"][0][2] == math.sqrt(w[29] / k)
    assert abs(math.sqrt(got[28] / k) - ref_run["history"][0][1]) <= (c[28] / 2 + 4) * U * ref_run["history"][0][1]
    M, g = P.normal_matrix(w)
    E, f = P.normal_matrix(e)
    x = P.plane_step(w)
    Minv = np.abs(np.linalg.inv(M))
    dx = Minv @ (f + E @ np.abs(x)) + 200 * U * (Minv @ (np.abs(M) @ np.abs(x)))
    cond = float(np.linalg.cond(np.outer(1 / np.sqrt(np.diag(M)), 1 / np.sqrt(np.diag(M))) * M))
    r_bound = math.sqrt(2.0) * float(np.linalg.norm(dx[:3])) + 16 * U
    lever = float(np.linalg.norm(pivot))
    t_bound = float(np.abs(dx[3:]).max()) + r_bound * lever + 16 * U * (lever + float(np.abs(x[3:]).max()))
    T, T_ref = CE.rigid_from_plane_moments(got, pivot), P.rigid_from_plane_moments(w, pivot)
    dR, dt = float(np.linalg.norm(T[:3, :3] - T_ref[:3, :3])), float(np.abs(T[:3, 3] - T_ref[:3, 3]).max())
    print(f"one plane iteration: cond(Ms) = {cond:.1f}; ||dR||_F = {dR:.2e} (bound {r_bound:.2e}); |dt| = {dt:.2e} (bound {t_bound:.2e})")
    RECORD["one_iteration"] = {"scaled_condition_number": cond, "rotation_difference": dR, "rotation_bound": r_bound, "translation_difference": dt,
                               "translation_bound": t_bound}
    assert dR <= r_bound and dt <= t_bound
    assert r_bound < 1e-10 and t_bound < 1e-7                 # (the bounds themselves say something)


# ---------------------------------------------------------------- the whole loop
_DEVICE_RUNS = {}


def device_run(dev, key):
    """"point": icp as it was; "analytic": method="plane" with case C's analytic normals; "estimated": with normals={"k": 20}"""
    from cer_mvs_amd import cloud_eval as CE
    if key not in _DEVICE_RUNS:
        src, dst, _, max_dist, _ = R.reference_run("C")
        s, d = on(dev, src), on(dev, dst)
        if key == "point":
            _DEVICE_RUNS[key] = CE.icp(s, d, max_dist)
        elif key == "analytic":
            _DEVICE_RUNS[key] = CE.icp(s, d, max_dist, method="plane", dst_normals=on(dev, P.reference_plane_run("analytic")[0]))
        else:
            _DEVICE_RUNS[key] = CE.icp(s, d, max_dist, method="plane", normals={"k": 20})
    return _DEVICE_RUNS[key]


def test_plane_icp_on_case_c_follows_the_restatement(dev):
    """the same iteration count, converged, fitness and pairs as the restatement; the device's T moves the points to within 1e-9 of the
    extent of where the restatement's does (3w's bar; expected: summation order alone); the planted motion to <= 0.02 float32 ulp"""
    from cer_mvs_amd import cloud_eval as CE
    src, dst, T_true, max_dist, _ = R.reference_run("C")
    nrm, ref = P.reference_plane_run("analytic")
    out = device_run(dev, "analytic")
    assert set(out) == {"T", "iterations", "converged", "fitness", "rmse", "rmse_point", "n_pairs", "history"}
    assert out["T"].dtype == np.float64 and out["T"].shape == (4, 4) and np.array_equal(out["T"][3], (0.0, 0.0, 0.0, 1.0))
    assert out["converged"] is True and ref["converged"] is True and out["iterations"] == ref["iterations"] == len(out["history"])
    assert out["n_pairs"] == ref["n_pairs"] and out["fitness"] == ref["fitness"]
    assert all(len(h) == 3 for h in out["history"]) and [h[0] for h in out["history"]] == [h[0] for h in ref["history"]]
    assert out["history"][-1] == (out["fitness"], out["rmse"], out["rmse_point"])
    assert out["iterations"] < device_run(dev, "point")["iterations"]
    bar = R.ulp32(np.abs(dst).max())
    planted = R.recovery_error(out["T"], T_true, src)
    to_ref = R.recovery_error(out["T"], ref["T"], src) / extent(dst)
    print(f"plane icp: {out['iterations']} iterations (point-to-point: {device_run(dev, 'point')['iterations']}); planted motion to {planted:.3e} "
          f"({planted / bar:.5f} ulp); restatement's T to {to_ref:.3e} of the extent")
    RECORD["icp_plane"] = {"iterations": out["iterations"], "iterations_point": device_run(dev, "point")["iterations"], "error_to_planted": planted,
                           "error_to_planted_ulps": planted / bar, "difference_to_restatement_over_extent": to_ref, "rmse": out["rmse"],
                           "rmse_point": out["rmse_point"]}
    assert to_ref <= 1e-9
    assert planted <= RECOVERY_ULPS * bar
    again = CE.icp(on(dev, src), on(dev, dst), max_dist, method="plane", dst_normals=on(dev, nrm))      # two runs: the same bits
    assert np.array_equal(again["T"].view(np.int64), out["T"].view(np.int64)) and again["history"] == out["history"]


def test_plane_icp_with_holes_in_the_normals(dev):
    """every 20th target normal (0, 0, 0): those matches make no pair - fitness exactly 0.95, as the restatement, and the loop converges"""
    from cer_mvs_amd import cloud_eval as CE
    src, dst, T_true, max_dist, _ = R.reference_run("C")
    nrm, ref = P.reference_plane_run("holes")
    out = CE.icp(on(dev, src), on(dev, dst), max_dist, method="plane", dst_normals=on(dev, nrm))
    assert out["converged"] and out["fitness"] == 0.95 == ref["fitness"] and out["iterations"] == ref["iterations"]
    assert R.recovery_error(out["T"], T_true, src) <= RECOVERY_ULPS * R.ulp32(np.abs(dst).max())


def test_plane_icp_with_normals_estimated_on_the_device(dev):
    """dst_normals=None: estimate_normals(dst, k=20), once; converges, in no more iterations than point-to-point, to the same bar"""
    from cer_mvs_amd import cloud_eval as CE
    src, dst, T_true, max_dist, _ = R.reference_run("C")
    out = device_run(dev, "estimated")
    bar = R.ulp32(np.abs(dst).max())
    err = R.recovery_error(out["T"], T_true, src)
    print(f"plane icp, estimated normals: {out['iterations']} iterations, fitness {out['fitness']}, planted motion to {err:.3e} ({err / bar:.5f} ulp)")
    RECORD["icp_plane_estimated_normals"] = {"iterations": out["iterations"], "fitness": out["fitness"], "error_to_planted": err,
                                             "error_to_planted_ulps": err / bar}
    assert out["converged"] and out["iterations"] <= device_run(dev, "point")["iterations"]
    assert err <= RECOVERY_ULPS * bar
    given = CE.icp(on(dev, src), on(dev, dst), max_dist, method="plane", dst_normals=CE.estimate_normals(on(dev, dst), k=20)[0])
    assert np.array_equal(given["T"].view(np.int64), out["T"].view(np.int64)) and given["history"] == out["history"]


def test_method_point_is_icp_as_it_was(dev):
    from cer_mvs_amd import cloud_eval as CE
    src, dst, _, max_dist, ref = R.reference_run("C")
    plain = device_run(dev, "point")
    named = CE.icp(on(dev, src), on(dev, dst), max_dist, method="point", dst_normals=None, normals=None)
    assert set(plain) == set(named) == {"T", "iterations", "converged", "fitness", "rmse", "n_pairs", "history"}
    assert np.array_equal(named["T"].view(np.int64), plain["T"].view(np.int64))
    assert {k: v for k, v in named.items() if k != "T"} == {k: v for k, v in plain.items() if k != "T"}
    assert plain["iterations"] == ref["iterations"] and all(len(h) == 2 for h in plain["history"])
    reg = CE.register(on(dev, src), on(dev, dst), [(None, max_dist, 50)], method="point")
    assert np.array_equal(reg["T"].view(np.int64), plain["T"].view(np.int64)) and reg["history"] == plain["history"]


def test_plane_icp_edges(dev):
    from cer_mvs_amd import cloud_eval as CE
    src, dst, T_true, max_dist, _ = R.reference_run("C")
    s, d, n = on(dev, src), on(dev, dst), on(dev, P.reference_plane_run("analytic")[0])
    init = R.motion((0, 1, 0), 0.1, (0.01, 0.0, 0.0), centre=src.astype(np.float64).mean(0))
    out = CE.icp(s, d, 1e-6, init=init, cell=0.25, method="plane", dst_normals=n)      # nothing within a millionth: fewer than 6 pairs
    assert out["n_pairs"] < 6 and out["converged"] is False and out["iterations"] == 1 and np.array_equal(out["T"], init)
    assert out["history"] == [(out["fitness"], out["rmse"], out["rmse_point"])]
    e = torch.empty(0, 3, device=dev)
    for a, b, nb in ((e, d, n), (s, e, e), (e, e, e), (e, d, None), (s, e, None)):
        out = CE.icp(a, b, max_dist, init=init, method="plane", dst_normals=nb)
        assert out["converged"] is False and out["iterations"] == 0 and out["n_pairs"] == 0 and out["history"] == [] and np.array_equal(out["T"], init)
        assert out["rmse_point"] == 0.0
    none = CE.icp(s, d, max_dist, method="plane", dst_normals=torch.zeros_like(n))    # no target has a plane: no pairs, T as it stands
    assert none["n_pairs"] == 0 and none["iterations"] == 1 and none["converged"] is False and np.array_equal(none["T"], np.eye(4))
    for bad in (n[:100], n[:, :2]):
        with pytest.raises(ValueError, match="dst_normals"):
            CE.icp(s, d, max_dist, method="plane", dst_normals=bad)
    with pytest.raises(RuntimeError, match="dst_normals"):
        CE.icp(s, d, max_dist, method="plane", dst_normals=n.double())
    with pytest.raises(ValueError, match="normals"):
        CE.icp(s, d, max_dist, method="plane", normals={"neighbours": 20})
    flat = torch.stack([s[:, 0], s[:, 1], 0.25 * s[:, 0] - 0.5 * s[:, 1]], 1).contiguous()      # a plane slides on itself
    fn = torch.tensor([-0.25, 0.5, 1.0], device=dev).div(math.sqrt(1.3125)).expand(len(src), 3).contiguous()
    with pytest.raises(ValueError, match="degenerate"):
        CE.icp(CE.rigid_transform(flat, R.motion((1, 0, 0), 0.0, (0.0, 0.0, 0.05))), flat, max_dist, method="plane", dst_normals=fn)


def test_register_plane_selects_the_normals_with_the_voxels(dev, monkeypatch):
    from cer_mvs_amd import cloud_eval as CE
    src, dst, T_true, max_dist, _ = R.reference_run("C")
    s, d, n = on(dev, src), on(dev, dst), on(dev, P.reference_plane_run("analytic")[0])
    seen, real_icp, real_estimate = [], CE.icp, CE.estimate_normals
    estimated = []

    def spy_icp(a, b, md, **kw):
        seen.append((b, kw.get("method"), kw.get("dst_normals")))
        return real_icp(a, b, md, **kw)

    def spy_estimate(points, **kw):
        estimated.append((int(points.shape[0]), kw))
        return real_estimate(points, **kw)
    monkeypatch.setattr(CE, "icp", spy_icp)
    monkeypatch.setattr(CE, "estimate_normals", spy_estimate)
    stages = ((4.0, 10.0, 30), (None, 5.0, 30))
    out = CE.register(s, d, stages, method="plane", dst_normals=n)
    sel = CE.voxel_downsample(d, 4.0)
    assert len(seen) == 2 and all(m == "plane" for _, m, _ in seen) and estimated == []
    assert torch.equal(seen[0][0], d.index_select(0, sel)) and torch.equal(seen[0][2], n.index_select(0, sel)) and len(sel) < len(dst)
    assert torch.equal(seen[1][0], d) and torch.equal(seen[1][2], n)
    assert len(out["stages"]) == 2 and out["converged"] and np.array_equal(out["T"], out["stages"][1]["T"]) and "rmse_point" in out
    assert out["stages"][0]["n_pairs"] < len(src) and out["n_pairs"] == len(src)
    err, bar = R.recovery_error(out["T"], T_true, src), R.ulp32(np.abs(dst).max())
    print(f"register(plane): stages of {[st['iterations'] for st in out['stages']]} iterations; planted motion to {err:.3e} ({err / bar:.5f} ulp)")
    RECORD["register_plane"] = {"iterations": [st["iterations"] for st in out["stages"]], "error_to_planted": err, "error_to_planted_ulps": err / bar}
    assert err <= RECOVERY_ULPS * bar
    del seen[:]
    out = CE.register(s, d, stages, method="plane", normals={"k": 20})                # estimated once, on the full cloud
    assert estimated == [(len(dst), {"k": 20})] and len(seen) == 2
    full = real_estimate(d, k=20)[0]
    assert torch.equal(seen[0][2], full.index_select(0, sel)) and torch.equal(seen[1][2], full)
    assert out["converged"] and R.recovery_error(out["T"], T_true, src) <= RECOVERY_ULPS * bar


# ---------------------------------------------------------------- the tool
def test_compare_clouds_tool_aligns_with_planes(dev, tmp_path):
    """a fresh child process per run: after --align icp-plane the F-score of the moved pair is that of the unmoved pair (dst against itself)"""
    from cer_mvs_amd.fusion import write_ply
    src, dst, T_true, max_dist, _ = R.reference_run("C")
    grey = np.full((len(src), 3), 128, np.uint8)
    write_ply(tmp_path / "a.ply", src, grey)
    write_ply(tmp_path / "b.ply", dst, grey)

    def run(a, *extra):
        res = subprocess.run([sys.executable, os.path.join(REPO, "tools", "compare_clouds.py"), str(tmp_path / a), str(tmp_path / "b.ply"),
                              "--max-dist", str(max_dist), "--tau", "0.05", *extra], capture_output=True, text=True, timeout=600, cwd=REPO)
        assert res.returncode == 0, res.stderr[-2000:]
        return json.loads(res.stdout.strip().splitlines()[-1])
    unmoved = run("b.ply")
    assert "align_method" not in unmoved and unmoved["fscore"] == 1.0
    got = run("a.ply", "--align", "icp-plane", "--align-normals-k", "20")
    from cer_mvs_amd import cloud_eval as CE
    info = {}
    CE.estimate_normals(on(dev, dst), k=20, info=info)        # a point of dst without a plane (the sparse rim) makes no pair; the matching is a bijection
    assert got["align_method"] == "plane" and got["align_converged"] is True
    assert got["align_fitness"] == info["n_valid"] / len(dst) > 0.99
    assert 0.0 <= got["align_rmse"] <= got["align_rmse_point"] * (1.0 + 1e-6) and got["align_rmse_point"] < 1e-4      # |D . n| <= |D| |n|, |n| = 1 in float32
    T = np.array(got["T"], np.float64)
    assert T.shape == (4, 4) and R.recovery_error(T, T_true, src) <= RECOVERY_ULPS * R.ulp32(np.abs(dst).max())
    assert got["fscore"] == unmoved["fscore"] and got["precision"] == unmoved["precision"] and got["recall"] == unmoved["recall"]
