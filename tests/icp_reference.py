"""A numpy fp64 restatement of the rigid registration in cer-mvs_amd/cloud_eval.py (csrc/cloud_align.hip), shared by
test_cloud_align_cpu.py and test_cloud_align_gpu.py: the transform with the kernel's association, a chunked brute-force nearest neighbour
with ``CloudIndex.nearest``'s contract, the 17 pair moments in numpy.longdouble, the Kabsch solve and the ICP loop with its stopping rule -
written here from the contract, importing nothing from the package - and the makers of the two registration cases."""
import math

import numpy as np

F32 = np.float32
LD = np.longdouble


# ---------------------------------------------------------------- the restatement
def transform(points, T):
    """float32 [n, 3]: float32(((T[r][0] * x + T[r][1] * y) + T[r][2] * z) + T[r][3]), x, y, z promoted to fp64 (numpy never fuses)"""
    P = np.asarray(points, F32).astype(np.float64).reshape(-1, 3)
    T = np.asarray(T, np.float64)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1).astype(F32)


def nearest(queries, target, max_dist, chunk=256):
    """-> (d2 float64 [m], idx int64 [m]): the target point with the smallest (d2, index), d2 = (dx*dx + dy*dy) + dz*dz in fp64, among those
    with d2 <= double(float32(max_dist))^2 (inclusive); (inf, -1) where there is none or the query is not finite; a non-finite target point
    is nobody's neighbour.  Brute force in chunks: the finite queries are grouped by the (x, y) cell of edge 2 max_dist they fall in, and a
    group is compared with every target point whose x and y lie within max_dist (and a margin) of the group's own bounding box, in the
    order of their indices - a point outside has |dx| or |dy| beyond max_dist and cannot be within it, so nothing rests on the cells."""
    Q = np.asarray(queries, F32).astype(np.float64).reshape(-1, 3)
    P = np.asarray(target, F32).astype(np.float64).reshape(-1, 3)
    md = np.float64(F32(max_dist))
    limit = md * md
    d2 = np.full(len(Q), np.inf)
    idx = np.full(len(Q), -1, np.int64)
    fin = np.flatnonzero(np.isfinite(Q).all(1))
    if not len(P) or not len(fin):
        return d2, idx
    reach = md * (1.0 + 1e-6) + 1e-300
    edge = max(2.0 * md, 1e-300)
    with np.errstate(invalid="ignore", over="ignore"):
        cells = np.floor(np.clip(Q[fin][:, :2] / edge, -1e15, 1e15))
        _, group = np.unique(cells, axis=0, return_inverse=True)
        group = group.reshape(-1)
        order = np.argsort(group, kind="stable")
        bounds = np.flatnonzero(np.diff(group[order], prepend=-1, append=group.max() + 1))
        for g0, g1 in zip(bounds[:-1], bounds[1:]):
            members = fin[order[g0:g1]]
            lo, hi = Q[members, :2].min(0) - reach, Q[members, :2].max(0) + reach
            cand = np.flatnonzero((P[:, 0] >= lo[0]) & (P[:, 0] <= hi[0]) & (P[:, 1] >= lo[1]) & (P[:, 1] <= hi[1]))      # ascending
            if not len(cand):
                continue
            C = P[cand]
            for s in range(0, len(members), chunk):
                qi = members[s:s + chunk]
                q = Q[qi]
                dx, dy, dz = C[None, :, 0] - q[:, None, 0], C[None, :, 1] - q[:, None, 1], C[None, :, 2] - q[:, None, 2]
                d = (dx * dx + dy * dy) + dz * dz
                d[~(d <= limit)] = np.inf                     # (NaN: a non-finite target point)
                j = d.argmin(1)                               # the first minimum: the lowest index on ties
                best = d[np.arange(len(q)), j]
                ok = np.isfinite(best)
                d2[qi] = np.where(ok, best, np.inf)
                idx[qi] = np.where(ok, cand[j], -1)
    return d2, idx


def nearest_plain(queries, target, max_dist, chunk=256):
    """the same contract with no grouping at all: every query against every target point (the tests check ``nearest`` against it)"""
    Q = np.asarray(queries, F32).astype(np.float64).reshape(-1, 3)
    P = np.asarray(target, F32).astype(np.float64).reshape(-1, 3)
    limit = np.float64(F32(max_dist)) * np.float64(F32(max_dist))
    d2 = np.full(len(Q), np.inf)
    idx = np.full(len(Q), -1, np.int64)
    if not len(P):
        return d2, idx
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, len(Q), chunk):
            q = Q[s:s + chunk]
            dx, dy, dz = P[None, :, 0] - q[:, None, 0], P[None, :, 1] - q[:, None, 1], P[None, :, 2] - q[:, None, 2]
            d = (dx * dx + dy * dy) + dz * dz
            d[~(d <= limit)] = np.inf
            j = d.argmin(1)
            best = d[np.arange(len(q)), j]
            ok = np.isfinite(best)
            d2[s:s + chunk] = np.where(ok, best, np.inf)
            idx[s:s + chunk] = np.where(ok, j, -1)
    return d2, idx


def moment_terms(a, b, idx, pivot=(0.0, 0.0, 0.0)):
    """the 17 columns of terms, one longdouble vector [k] at a time, of the pairs (a[i], b[idx[i]]), idx[i] >= 0 and a[i] finite, in the order
    of i: 1 | A | B | A[r] * B[c] at 7 + 3 r + c | (Dx*Dx + Dy*Dy) + Dz*Dz, with A = a - pivot, B = b - pivot, D = a - b"""
    a, b, idx = np.asarray(a, F32).reshape(-1, 3), np.asarray(b, F32).reshape(-1, 3), np.asarray(idx, np.int64)
    sel = (idx >= 0) & np.isfinite(a).all(1)
    pa, pb = a[sel].astype(LD), b[idx[sel]].astype(LD)
    piv = np.asarray(pivot, np.float64).astype(LD)
    A, B, D = pa - piv, pb - piv, pa - pb
    yield np.ones(len(A), LD)
    for M in (A, B):
        for r in range(3):
            yield np.ascontiguousarray(M[:, r])
    for r in range(3):
        for c in range(3):
            yield A[:, r] * B[:, c]
    yield (D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2]


def moments(a, b, idx, pivot=(0.0, 0.0, 0.0), with_magnitude=False):
    """longdouble [17] (and, on request, the sums of the terms' magnitudes).  Every column is summed on its own as a contiguous vector: numpy's
    pairwise summation, whose error is a few dozen roundings of 2^-64 - 1e-2 of one fp64 rounding."""
    s, mag = np.zeros(17, LD), np.zeros(17, LD)
    for k, t in enumerate(moment_terms(a, b, idx, pivot)):
        s[k] = np.sum(t)
        if with_magnitude:
            mag[k] = np.sum(np.abs(t))
    return (s, mag) if with_magnitude else s


def rigid_from_moments(mom, pivot=(0.0, 0.0, 0.0)):
    """Kabsch on the 17 sums -> 4x4 float64: H = sum A x B - k Abar x Bbar = U S V^T, R = V diag(1, 1, det(V U^T)) U^T, t = (Bbar + pivot) -
    R (Abar + pivot); ValueError for k < 3 and for collinear pairs (S[1] <= 1e-12 S[0])"""
    mom, pivot = np.asarray(mom, np.float64), np.asarray(pivot, np.float64)
    k = mom[0]
    if not k >= 3:
        raise ValueError("fewer than 3 pairs")
    abar, bbar = mom[1:4] / k, mom[4:7] / k
    H = mom[7:16].reshape(3, 3) - k * np.outer(abar, bbar)
    U, S, Vt = np.linalg.svd(H)
    if not S[1] > 1e-12 * S[0]:
        raise ValueError("collinear pairs")
    V = Vt.T
    R = V @ np.diag((1.0, 1.0, float(np.sign(np.linalg.det(V @ U.T))))) @ U.T
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = (bbar + pivot) - R @ (abar + pivot)
    return T


def icp(src, dst, max_dist, init=None, max_iter=50, tol_fitness=1e-6, tol_rmse=1e-6, pivot=None):
    """The loop of cloud_eval.icp.  ``pivot`` defaults to the per-axis minimum of the finite ``dst`` points (the grid's origin)."""
    src, dst = np.asarray(src, F32).reshape(-1, 3), np.asarray(dst, F32).reshape(-1, 3)
    T = np.eye(4) if init is None else np.array(init, np.float64)
    out = {"T": T, "iterations": 0, "converged": False, "fitness": 0.0, "rmse": 0.0, "n_pairs": 0, "history": []}
    finite = np.isfinite(dst).all(1)
    if not len(src) or not finite.any():
        return out
    if pivot is None:
        pivot = dst[finite].min(0).astype(np.float64)
    for _ in range(max_iter):
        cur = transform(src, T)
        mom = moments(cur, dst, nearest(cur, dst, max_dist)[1], pivot).astype(np.float64)
        k = int(mom[0])
        fitness, rmse = k / len(src), (math.sqrt(mom[16] / k) if k else 0.0)
        moved = (abs(fitness - out["fitness"]), abs(rmse - out["rmse"])) if out["iterations"] else None
        out["history"].append((fitness, rmse))
        out.update(iterations=out["iterations"] + 1, fitness=fitness, rmse=rmse, n_pairs=k)
        if k < 3:
            break
        if moved is not None and moved[0] < tol_fitness and moved[1] < tol_rmse:
            out["converged"] = True
            break
        T = rigid_from_moments(mom, pivot) @ T
        out["T"] = T
    return out


# ---------------------------------------------------------------- motions and cases
def motion(axis, degrees, translation, centre=(0.0, 0.0, 0.0)):
    """4x4 float64: the rotation by ``degrees`` about ``axis`` through ``centre`` (Rodrigues), then ``translation``"""
    u = np.asarray(axis, np.float64)
    u = u / np.linalg.norm(u)
    K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    th = math.radians(degrees)
    R = np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)
    c = np.asarray(centre, np.float64)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = c - R @ c + np.asarray(translation, np.float64)
    return T


def apply64(T, P):
    """fp64 [n, 3]: T applied to P without the rounding to float32"""
    return np.asarray(P, np.float64) @ np.asarray(T, np.float64)[:3, :3].T + np.asarray(T, np.float64)[:3, 3]


def case_a():
    """-> (src, dst float32, T_true, max_dist): a 16^3 unit lattice jittered by +-0.2 and offset by (100, -50, 300); dst its image under 0.4
    degrees about (1, 2, 3) through the centroid plus (0.05, -0.08, 0.06), rounded to float32 and shuffled.  Every point moves by less than
    0.2 - under half the minimum spacing of 0.6 - so every first match is the right one."""
    rng = np.random.default_rng(101)
    g = np.arange(16, dtype=np.float64)
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + rng.uniform(-0.2, 0.2, (4096, 3)) + np.array([100.0, -50.0, 300.0])
    src = P.astype(F32)
    T = motion((1, 2, 3), 0.4, (0.05, -0.08, 0.06), centre=src.astype(np.float64).mean(0))
    dst = apply64(T, src)[rng.permutation(len(src))].astype(F32)
    return src, dst, T, 0.5


def case_c():
    """-> (src, dst float32, T_true, max_dist): 20 000 points of z = 0.3 sin 3u cos 2v + 0.1 u^2 + 0.15 sin 7v over (u, v) in [-1, 1]^2, scaled
    by 50 and offset by (10, 20, 500); dst its shuffled image under 3 degrees about (0.3, 1, 0.5) through the centroid plus (1, -0.7, 0.5)"""
    rng = np.random.default_rng(303)
    u, v = rng.uniform(-1.0, 1.0, 20000), rng.uniform(-1.0, 1.0, 20000)
    z = 0.3 * np.sin(3 * u) * np.cos(2 * v) + 0.1 * u * u + 0.15 * np.sin(7 * v)
    src = (50.0 * np.stack([u, v, z], 1) + np.array([10.0, 20.0, 500.0])).astype(F32)
    T = motion((0.3, 1, 0.5), 3.0, (1.0, -0.7, 0.5), centre=src.astype(np.float64).mean(0))
    dst = apply64(T, src)[rng.permutation(len(src))].astype(F32)
    return src, dst, T, 5.0


CASES = {"A": case_a, "C": case_c}
_RUNS = {}


def reference_run(name):
    """(src, dst, T_true, max_dist, the restatement's icp dict) of a case - computed once per process, shared by the tests, never modified"""
    if name not in _RUNS:
        src, dst, T, max_dist = CASES[name]()
        for arr in (src, dst, T):
            arr.setflags(write=False)
        _RUNS[name] = (src, dst, T, max_dist, icp(src, dst, max_dist))
    return _RUNS[name]


def ulp32(x):
    """one float32 ulp at magnitude x"""
    return float(np.spacing(F32(abs(x))))


def recovery_error(T, T_true, points):
    """max over the points and the axes of |T p - T_true p|, fp64"""
    return float(np.abs(apply64(T, points) - apply64(T_true, points)).max())
