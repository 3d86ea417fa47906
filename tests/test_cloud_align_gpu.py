"""Rigid registration on the MI355X (csrc/cloud_align.hip, cer-mvs_amd/cloud_eval.py) against the numpy restatement of
tests/icp_reference.py.

The transform must equal the restatement bit for bit (same association, no fused multiply-add, one rounding to float32).

The moments: with small-integer coordinates and an integer pivot every term and every partial sum is an integer below 2^53, so whatever the
summation order all 17 sums are exact and must equal the restatement bit for bit - any indexing error shows without a tolerance.  With
float coordinates sum k must lie within c_k * 2^-53 * sum|term| of the longdouble reference, c_k counted from the kernel's own shape
(u = 2^-53; a sum of n additions along the deepest path of its tree errs by at most n u sum|term| to first order):
    roundings of a term   count 0 (the term is 1); sum A, sum B 1 (the subtraction of the pivot); A[r] * B[c] 3 (two subtractions, one product);
                          d2 5 (D = a - b 1, squared 2 + 1, two additions of non-negative products 2)
    pass 1                a thread's MOMENT_TILE / 256 = 8 terms in sequence: 8 additions (the first, onto 0, is exact: one to spare); the
                          butterfly over 64 lanes 6; four waves as (w0 + w1) + (w2 + w3): 2
    pass 2                ceil(P / 1024) partials per thread in sequence, P = ceil(m / MOMENT_TILE); butterfly 6; sixteen waves pairwise 4
    the reference         1 (numpy's pairwise longdouble sum: 1e-2 of one fp64 rounding; the rest is to spare)
so c_k = term_k + 8 + 6 + 2 + ceil(P / 1024) + 6 + 4 + 1, times (1 + 64 u) for the second-order terms.

The loop: cases A and C of icp_reference.py.  Measured maxima go to profiles/cloud_align_parity.json under CER_PARITY_RECORD=1 (a run of the
whole module); a plain run writes nothing.  Measured on an MI355X: moments, largest |err| / bound over the sizes 0.054; one iteration on case C,
rotation 6.2e-16 against a bound of 1.7e-13, translation 1.7e-13 against 8.5e-11; cases A / C: 4 / 12 iterations, the planted motion to 6.1e-8 /
3.4e-8 (0.002 / 0.0006 of the bar), the restatement's T to 3.7e-15 / 2.2e-15 of the extent; register 28 + 7 iterations, 1.6e-8."""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import icp_reference as R
from conftest import REPO

pytestmark = pytest.mark.gpu

F32 = np.float32
U = 2.0 ** -53
TERM_ROUNDINGS = np.array([0] + [1] * 6 + [3] * 9 + [5], np.float64)
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
        path = os.path.join(REPO, "profiles", "cloud_align_parity.json") if target == "1" else target
        with open(path, "w") as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
            f.write("\n")


def bits(x):
    return np.ascontiguousarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x, F32).view(np.int32)


def on(dev, array):
    """a tensor on the device with a copy of ``array`` (the shared cases are read-only)"""
    return torch.from_numpy(np.array(array)).to(dev)


def general_motion():
    return R.motion((0.3, -1.0, 0.45), 37.0, (12.5, -3.25, 700.125), centre=(5.0, 6.0, 7.0))


# ---------------------------------------------------------------- transform
def raw_transform(dev, pts, T):
    """the entry point itself, into a NaN-filled buffer"""
    from cer_mvs_amd import _lib as L
    p = torch.from_numpy(np.ascontiguousarray(pts, F32)).to(dev)
    out = torch.full((len(pts), 3), float("nan"), device=dev)
    rows = (ctypes.c_double * 12)(*[float(v) for v in np.asarray(T, np.float64)[:3].reshape(-1)])
    L.check(L.load().cer_cloud_transform_f32(L.dev_ptr(p, "points"), len(pts), rows, L.dev_ptr(out, "out"), L.cur_stream()), "cloud_transform")
    return out.cpu().numpy()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_transform_equals_the_restatement_bit_for_bit(dev, n):
    from cer_mvs_amd import cloud_eval as CE
    rng = np.random.default_rng(n)
    pts = (rng.uniform(-100.0, 100.0, (n, 3)) + np.array([10.0, 20.0, 500.0])).astype(F32)
    T = general_motion()
    want = R.transform(pts, T)
    got = raw_transform(dev, pts, T)
    assert np.isfinite(got).all()                             # every output written
    assert np.array_equal(bits(got), bits(want))
    via = CE.rigid_transform(torch.from_numpy(pts).to(dev), T)
    assert via.dtype == torch.float32 and tuple(via.shape) == (n, 3) and np.array_equal(bits(via), bits(want))
    assert np.array_equal(bits(CE.rigid_transform(torch.from_numpy(pts).to(dev), torch.from_numpy(T))), bits(want))      # T as a tensor
    ident = raw_transform(dev, pts, np.eye(4))               # (1 * x + 0 * y) + 0 * z + 0 = x for every finite x but -0.0
    assert np.array_equal(bits(ident), bits(pts))


def test_transform_of_non_finite_and_huge_rows_follows_ieee(dev):
    rng = np.random.default_rng(7)
    pts = rng.uniform(-10.0, 10.0, (300, 3)).astype(F32)
    pts[3, 0], pts[64, 1], pts[65, 2], pts[130] = np.nan, np.inf, -np.inf, (np.inf, -np.inf, 1.0)
    pts[200], pts[201, 1], pts[255] = 1e30, -1e30, (3e38, 3e38, 3e38)
    for T in (general_motion(), np.eye(4), R.motion((0, 0, 1), 90.0, (0, 0, 0))):
        want, got = R.transform(pts, T), raw_transform(dev, pts, T)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.array_equal(bits(got)[ok], bits(want)[ok])
    assert np.isnan(want).any() and np.isinf(want).any()


def test_transform_of_an_empty_cloud(dev):
    from cer_mvs_amd import cloud_eval as CE
    out = CE.rigid_transform(torch.empty(0, 3, device=dev), general_motion())
    assert tuple(out.shape) == (0, 3) and out.dtype == torch.float32


# ---------------------------------------------------------------- moments
def moment_sizes():
    from cer_mvs_amd import cloud_eval as CE
    tile = CE.MOMENT_TILE
    return [1, 255, 256, 257, tile + 1, 1024 * tile + 1]     # the last: 1025 partials, one more than the second pass's block is wide


def moment_case(m, integer, seed):
    """a, b, idx: a random map into 1000 target points with about a quarter -1 and a few non-finite rows of a"""
    rng = np.random.default_rng(seed)
    nb = 1000
    if integer:
        a, b = rng.integers(-60, 61, (m, 3)).astype(F32), rng.integers(-60, 61, (nb, 3)).astype(F32)
        pivot = (-7.0, 11.0, 3.0)
    else:
        a = (rng.uniform(-40.0, 40.0, (m, 3)) + np.array([10.0, 20.0, 500.0])).astype(F32)
        b = (rng.uniform(-40.0, 40.0, (nb, 3)) + np.array([10.0, 20.0, 500.0])).astype(F32)
        pivot = (-30.0, -20.0, 460.0)
    idx = rng.integers(0, nb, m)
    idx[rng.uniform(size=m) < 0.25] = -1
    idx[0] = idx[0] if m > 1 else 0                           # (the single pair is a pair)
    for j, v in zip(rng.integers(0, m, min(m // 50, 7)), (np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan, np.nan)):
        a[j, rng.integers(0, 3)] = v
    return a, b, idx.astype(np.int64), pivot


def device_moments(dev, a, b, idx, pivot):
    from cer_mvs_amd import cloud_eval as CE
    return CE.pair_moments(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), torch.from_numpy(idx).to(dev), pivot)


def moment_constants(m):
    from cer_mvs_amd import _lib as L
    from cer_mvs_amd import cloud_eval as CE
    P = int(L.load().cer_cloud_moment_partials(m))
    assert P == -(-m // CE.MOMENT_TILE)
    return (TERM_ROUNDINGS + (CE.MOMENT_TILE // 256 + 6 + 2) + (-(-P // 1024) + 6 + 4) + 1) * (1.0 + 64 * U), P


@pytest.mark.parametrize("m", moment_sizes())
def test_moments_of_integer_coordinates_are_exact(dev, m):
    a, b, idx, pivot = moment_case(m, True, seed=m)
    want = R.moments(a, b, idx, pivot)
    assert float(np.abs(want).max()) < 2.0 ** 53
    got = device_moments(dev, a, b, idx, pivot)
    assert got.dtype == np.float64 and got.shape == (17,)
    assert got[0] == np.count_nonzero((idx >= 0) & np.isfinite(a).all(1))
    assert np.array_equal(got, want.astype(np.float64)), (got - want.astype(np.float64))
    assert np.array_equal(got.view(np.int64), device_moments(dev, a, b, idx, pivot).view(np.int64))      # two launches


@pytest.mark.parametrize("m", moment_sizes())
def test_moments_of_float_coordinates_are_within_the_counted_bound(dev, m):
    a, b, idx, pivot = moment_case(m, False, seed=m + 1)
    want, mag = R.moments(a, b, idx, pivot, with_magnitude=True)
    c, P = moment_constants(m)
    got = device_moments(dev, a, b, idx, pivot)
    assert got[0] == float(want[0])                           # k is exact
    err = np.abs(got.astype(np.longdouble) - want)
    bound = c.astype(np.longdouble) * U * mag
    ratio = float((err[1:] / bound[1:]).max()) if want[0] else 0.0
    print(f"m = {m}: {P} partials, k = {int(got[0])}, max |err| / bound = {ratio:.3f}")
    RECORD.setdefault("moments_max_err_over_bound", {})[str(m)] = ratio
    assert (err <= bound).all(), (err / np.maximum(bound, np.longdouble(1e-300))).astype(np.float64)
    again = device_moments(dev, a, b, idx, pivot)
    assert np.array_equal(got.view(np.int64), again.view(np.int64))
    plain = device_moments(dev, a, b, idx, None)              # the default pivot is the origin
    assert np.array_equal(plain.view(np.int64), device_moments(dev, a, b, idx, (0.0, 0.0, 0.0)).view(np.int64))
    if P == 2:                                                # what the pivot is for: without one the covariance terms are 100 times the size
        assert R.moments(a, b, idx, (0.0, 0.0, 0.0), with_magnitude=True)[1][15] > 50 * mag[15]


def test_moments_without_pairs_are_zero(dev):
    from cer_mvs_amd import cloud_eval as CE
    a, b, idx, pivot = moment_case(3000, False, seed=9)
    none = np.full_like(idx, -1)
    got = device_moments(dev, a, b, none, pivot)
    assert np.array_equal(got, np.zeros(17)) and not np.signbit(got).any()
    a[:] = np.nan                                             # every a non-finite: no pair either
    assert np.array_equal(device_moments(dev, a, b, np.abs(idx), pivot), np.zeros(17))
    e = torch.empty(0, 3, device=dev)
    assert np.array_equal(CE.pair_moments(e, torch.from_numpy(b).to(dev), torch.empty(0, dtype=torch.int64, device=dev)), np.zeros(17))
    p = torch.from_numpy(b).to(dev)
    for bad in (torch.full((1000,), 1000, dtype=torch.int64), torch.full((1000,), -2, dtype=torch.int64), torch.zeros(999, dtype=torch.int64),
                torch.zeros(1000, dtype=torch.int32)):
        with pytest.raises(ValueError, match="idx"):
            CE.pair_moments(p, p, bad.to(dev))


# ---------------------------------------------------------------- one iteration
def test_one_iteration_on_case_c(dev):
    """at T = I: the matches are the restatement's, fitness is equal, and rmse and the new T are within the moments' bound propagated:
      rmse = sqrt(m16 / k): m16 is a sum of non-negative terms, relative error <= c16 u; the division and the root add a rounding each on
        both sides: |rmse - ref| <= (c16 / 2 + 4) u rmse.
      T: H = sum A x B - sum A (sum B)^T / k moves by at most e_H = e[7:16] + (e[1:4] |sum B|^T + |sum A| e[4:7]^T) / k entry by entry
        (e = the moments' bounds; three more roundings of each entry's own magnitude for the centring itself), and both solves add the
        backward error of LAPACK's 3 x 3 SVD and of the three 3 x 3 products behind R - taken as 100 u ||H||_F, ten times the textbook
        constant.  The rotation factor of a matrix moves by at most 2 ||dH||_F / (s2 + s3) (the polar factor's perturbation bound; s: H's
        singular values), so ||dR||_F <= 2 (||e_H||_F + 100 u ||H||_F) / (s2 + s3) =: r, and t = (Bbar + p) - R (Abar + p) by at most
        (e[1:4] + e[4:7]) / k + r |Abar + p| + 8 u (|Bbar + p| + |Abar + p|)."""
    from cer_mvs_amd import cloud_eval as CE
    src, dst, T_true, max_dist, ref_run = R.reference_run("C")
    s, d = on(dev, src), on(dev, dst)
    index = CE.CloudIndex(d, max_dist / CE.DEFAULT_CELL_DIVISOR)
    cur = CE.rigid_transform(s, np.eye(4))
    assert np.array_equal(bits(cur), bits(src))
    dist, idx = index.nearest(cur, max_dist)
    d2_ref, idx_ref = R.nearest(src, dst, max_dist)
    assert np.array_equal(idx.cpu().numpy(), idx_ref)
    pivot = np.array([float(v) for v in index.origin])
    assert np.array_equal(pivot, dst.min(0).astype(np.float64))
    got = CE.pair_moments(cur, d, idx, pivot)
    want, mag = R.moments(src, dst, idx_ref, pivot, with_magnitude=True)
    c, _ = moment_constants(len(src))
    e = (c * U * mag.astype(np.float64))
    assert (np.abs(got.astype(np.longdouble) - want) <= c.astype(np.longdouble) * U * mag).all()
    k = int(got[0])
    assert k == int(want[0]) == np.count_nonzero(idx_ref >= 0) and k / len(src) == ref_run["history"][0][0]
    w = want.astype(np.float64)
    rmse, rmse_ref = math.sqrt(got[16] / k), ref_run["history"][0][1]
    assert rmse_ref == math.sqrt(w[16] / k)
    assert abs(rmse - rmse_ref) <= (c[16] / 2 + 4) * U * rmse_ref
    T, T_ref = CE.rigid_from_moments(got, pivot), R.rigid_from_moments(w, pivot)
    abar, bbar = w[1:4] / k, w[4:7] / k
    H = w[7:16].reshape(3, 3) - k * np.outer(abar, bbar)
    e_H = e[7:16].reshape(3, 3) + (np.outer(e[1:4], np.abs(w[4:7])) + np.outer(np.abs(w[1:4]), e[4:7])) / k \
        + 3 * U * (np.abs(w[7:16]).reshape(3, 3) + k * np.outer(np.abs(abar), np.abs(bbar)))
    sv = np.linalg.svd(H, compute_uv=False)
    r = 2.0 * (np.linalg.norm(e_H) + 100 * U * np.linalg.norm(H)) / (sv[1] + sv[2])
    lever_a, lever_b = np.linalg.norm(abar + pivot), np.linalg.norm(bbar + pivot)
    t_bound = float((e[1:4] + e[4:7]).max()) / k + r * lever_a + 8 * U * (lever_a + lever_b)
    dR, dt = float(np.linalg.norm(T[:3, :3] - T_ref[:3, :3])), float(np.abs(T[:3, 3] - T_ref[:3, 3]).max())
    print(f"one iteration: |rmse - ref| / rmse = {abs(rmse - rmse_ref) / rmse_ref:.2e}; ||dR||_F = {dR:.2e} (bound {r:.2e}); |dt| = {dt:.2e} (bound {t_bound:.2e})")
    RECORD["one_iteration"] = {"rotation_difference": dR, "rotation_bound": r, "translation_difference": dt, "translation_bound": t_bound}
    assert dR <= r and dt <= t_bound
    assert r < 1e-10 and t_bound < 1e-8                      # (the bounds themselves say something)


# ---------------------------------------------------------------- the whole loop
_DEVICE_RUNS = {}


def device_run(dev, name):
    from cer_mvs_amd import cloud_eval as CE
    if name not in _DEVICE_RUNS:
        src, dst, _, max_dist, _ = R.reference_run(name)
        _DEVICE_RUNS[name] = CE.icp(on(dev, src), on(dev, dst), max_dist)
    return _DEVICE_RUNS[name]


def extent(points):
    return float((points.max(0).astype(np.float64) - points.min(0).astype(np.float64)).max())


@pytest.mark.parametrize("name", ["A", "C"])
def test_icp_recovers_the_planted_motion_like_the_restatement(dev, name):
    """the same iteration count as the restatement and converged; for every point p of the cloud |T p - T_true p| <= 1 float32 ulp of the
    largest |coordinate| of dst; against the restatement's T, 1e-9 of the extent (expected: 1e-13 of it, from summation order alone)"""
    from cer_mvs_amd import cloud_eval as CE
    src, dst, T_true, max_dist, ref = R.reference_run(name)
    out = device_run(dev, name)
    assert set(out) == {"T", "iterations", "converged", "fitness", "rmse", "n_pairs", "history"}
    assert out["T"].dtype == np.float64 and out["T"].shape == (4, 4) and np.array_equal(out["T"][3], (0.0, 0.0, 0.0, 1.0))
    assert out["converged"] is True and out["iterations"] == ref["iterations"] == len(out["history"])
    assert out["n_pairs"] == ref["n_pairs"] and out["fitness"] == ref["fitness"]
    assert [h[0] for h in out["history"]] == [h[0] for h in ref["history"]]
    bar = R.ulp32(np.abs(dst).max())
    planted = R.recovery_error(out["T"], T_true, src)
    ext = extent(dst)
    to_ref = R.recovery_error(out["T"], ref["T"], src) / ext
    rmse_gap = max(abs(a[1] - b[1]) for a, b in zip(out["history"], ref["history"]))
    print(f"case {name}: {out['iterations']} iterations; planted motion to {planted:.3e} ({planted / bar:.4f} of the bar); "
          f"restatement's T to {to_ref:.3e} of the extent; largest rmse gap {rmse_gap:.3e}")
    RECORD.setdefault("icp", {})[name] = {"iterations": out["iterations"], "error_to_planted": planted, "error_to_planted_over_bar": planted / bar,
                                          "difference_to_restatement_over_extent": to_ref, "largest_rmse_gap": rmse_gap, "rmse": out["rmse"]}
    assert planted <= bar
    assert to_ref <= 1e-9
    again = CE.icp(on(dev, src), on(dev, dst), max_dist)      # two runs: the same bits
    assert np.array_equal(again["T"].view(np.int64), out["T"].view(np.int64)) and again["history"] == out["history"]
    assert again["iterations"] == out["iterations"]


def test_icp_edges(dev):
    from cer_mvs_amd import cloud_eval as CE
    src, dst, T_true, max_dist, _ = R.reference_run("A")
    s, d = on(dev, src), on(dev, dst)
    init = R.motion((0, 1, 0), 0.1, (0.01, 0.0, 0.0), centre=src.astype(np.float64).mean(0))
    out = CE.icp(s, d, 1e-6, init=init, cell=0.25)           # nothing within a millionth: fewer than 3 pairs
    assert out["n_pairs"] < 3 and out["converged"] is False and out["iterations"] == 1 and np.array_equal(out["T"], init)
    assert out["history"] == [(out["fitness"], out["rmse"])]
    e = torch.empty(0, 3, device=dev)
    for a, b in ((e, d), (s, e), (e, e), (s, torch.full((5, 3), float("nan"), device=dev))):
        out = CE.icp(a, b, max_dist, init=init)
        assert out["converged"] is False and out["iterations"] == 0 and out["n_pairs"] == 0 and out["history"] == [] and np.array_equal(out["T"], init)
    with pytest.raises(ValueError, match="index"):
        CE.icp(s, d, max_dist, index=CE.CloudIndex(d[:100].contiguous(), 0.25))
    with pytest.raises(ValueError, match="index"):
        CE.icp(s, d, max_dist, index="grid")
    one = CE.icp(s, d, max_dist, max_iter=1)                 # the loop is bounded by max_iter
    assert one["iterations"] == 1 and one["converged"] is False and not np.array_equal(one["T"], np.eye(4))


def test_icp_from_the_planted_motion_and_with_a_reused_index(dev):
    from cer_mvs_amd import cloud_eval as CE
    src, dst, T_true, max_dist, _ = R.reference_run("C")
    s, d = on(dev, src), on(dev, dst)
    out = CE.icp(s, d, max_dist, init=T_true)
    assert out["converged"] and out["iterations"] <= 3
    assert R.recovery_error(out["T"], T_true, src) <= R.ulp32(np.abs(dst).max())
    index = CE.CloudIndex(d, max_dist / CE.DEFAULT_CELL_DIVISOR)
    built = device_run(dev, "C")
    for _ in range(2):                                        # the index is not consumed
        reused = CE.icp(s, d, max_dist, index=index)
        assert np.array_equal(reused["T"].view(np.int64), built["T"].view(np.int64)) and reused["history"] == built["history"]
    coarse = CE.icp(s, d, max_dist, cell=max_dist)            # another grid, another pivot: the same motion to the bar
    assert coarse["converged"] and R.recovery_error(coarse["T"], T_true, src) <= R.ulp32(np.abs(dst).max())


def test_register_coarse_to_fine_on_case_c(dev):
    from cer_mvs_amd import cloud_eval as CE
    src, dst, T_true, max_dist, _ = R.reference_run("C")
    s, d = on(dev, src), on(dev, dst)
    out = CE.register(s, d, ((4.0, 10.0, 30), (None, 5.0, 30)))
    assert len(out["stages"]) == 2 and out["converged"] and np.array_equal(out["T"], out["stages"][1]["T"])
    assert out["stages"][0]["n_pairs"] < len(src) and out["n_pairs"] == len(src)      # the first stage ran on the thinned clouds
    assert out["stages"][1]["iterations"] < device_run(dev, "C")["iterations"]        # and left the second less to do
    err, bar = R.recovery_error(out["T"], T_true, src), R.ulp32(np.abs(dst).max())
    print(f"register: stages of {[st['iterations'] for st in out['stages']]} iterations; planted motion to {err:.3e} ({err / bar:.4f} of the bar)")
    RECORD["register"] = {"iterations": [st["iterations"] for st in out["stages"]], "error_to_planted": err, "error_to_planted_over_bar": err / bar}
    assert err <= bar
    same = CE.register(s, d, [(None, 5.0, 50)])
    assert np.array_equal(same["T"].view(np.int64), device_run(dev, "C")["T"].view(np.int64))       # one full stage is icp itself


# ---------------------------------------------------------------- align= and the tool
def test_align_argument_of_the_protocols(dev):
    from cer_mvs_amd import cloud_eval as CE
    src, dst, T_true, max_dist, _ = R.reference_run("A")
    s, d = on(dev, src), on(dev, dst)
    T = device_run(dev, "A")["T"]
    moved = CE.rigid_transform(s, T)
    tau = 0.05
    assert CE.fscore(s, d, tau, align=T) == CE.fscore(moved, d, tau)
    assert CE.fscore(s, d, tau, align=None) == CE.fscore(s, d, tau)
    assert CE.fscore(s, d, tau, align=T)["fscore"] == 1.0 and CE.fscore(s, d, tau)["fscore"] < 0.5
    keep = torch.arange(len(src), device=dev) % 3 != 0
    for kw in ({}, {"thin": 1.5}, {"thin": 1.5, "thin_method": "greedy"}, {"keep_pred": keep}):
        a, b = CE.accuracy_completeness(s, d, max_dist=max_dist, align=T, **kw), CE.accuracy_completeness(moved, d, max_dist=max_dist, **kw)
        assert a == b and a["n_pred_in"] > 0
        a, b = CE.accuracy_completeness(s, d, max_dist=max_dist, align=None, **kw), CE.accuracy_completeness(s, d, max_dist=max_dist, **kw)
        assert a == b and a["n_pred_in"] > 0
    assert CE.accuracy_completeness(s, d, max_dist=max_dist, align=T)["accuracy"] < 1e-5


def test_compare_clouds_tool_aligns(dev, tmp_path):
    """a fresh child process: --align icp reports a T that meets the recovery bar, and F is at least what --align none gives"""
    from cer_mvs_amd.fusion import write_ply
    src, dst, T_true, max_dist, _ = R.reference_run("A")
    grey = np.full((len(src), 3), 128, np.uint8)
    write_ply(tmp_path / "a.ply", src, grey)
    write_ply(tmp_path / "b.ply", dst, grey)
    np.savetxt(tmp_path / "init.txt", np.eye(4))

    def run(*extra):
        res = subprocess.run([sys.executable, os.path.join(REPO, "tools", "compare_clouds.py"), str(tmp_path / "a.ply"), str(tmp_path / "b.ply"),
                              "--max-dist", str(max_dist), "--tau", "0.05", *extra], capture_output=True, text=True, timeout=600, cwd=REPO)
        assert res.returncode == 0, res.stderr[-2000:]
        return json.loads(res.stdout.strip().splitlines()[-1])
    plain = run()
    assert "T" not in plain and "align_iterations" not in plain
    got = run("--align", "icp", "--init", str(tmp_path / "init.txt"), "--align-voxel", "0.5", "--align-max-dist", str(max_dist))
    T = np.array(got["T"], np.float64)
    assert T.shape == (4, 4) and np.array_equal(T[3], (0.0, 0.0, 0.0, 1.0))
    assert R.recovery_error(T, T_true, src) <= R.ulp32(np.abs(dst).max())
    assert got["align_iterations"] >= 2 and got["align_fitness"] == 1.0 and got["align_rmse"] < 1e-5
    assert got["fscore"] >= plain["fscore"] and got["fscore"] == 1.0 and plain["fscore"] < 0.5
