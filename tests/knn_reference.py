"""A numpy fp64 restatement of the k-nearest search, the count within a radius and the two outlier filters of cer-mvs_amd/cloud_eval.py
(csrc/cloud_eval.hip grid_knn_kernel / grid_count_within_kernel), shared by test_cloud_knn_cpu.py and test_cloud_knn_gpu.py.
Written here from the contract, importing nothing from the package: a brute force in 256-query chunks with the same three operations for d2,
non-finite values set to inf, a stable argsort (the lowest index first on ties), the <= test against double(float32(max_dist))^2,
np.float32(np.sqrt(d2)), and the mean as a sequential sum in ascending order."""
import numpy as np

F32 = np.float32
KNN_MAX = 32


def _clouds(target, queries):
    return (np.asarray(target, F32).astype(np.float64).reshape(-1, 3), np.asarray(queries, F32).astype(np.float64).reshape(-1, 3))


def _d2(T, q):
    """[len(q), len(T)] fp64: (dx*dx + dy*dy) + dz*dz; inf where a point or a query is not finite"""
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = T[None, :, 0] - q[:, None, 0], T[None, :, 1] - q[:, None, 1], T[None, :, 2] - q[:, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
    return np.where(np.isfinite(d2), d2, np.inf)


def limit_of(max_dist):
    return np.float64(F32(max_dist)) * np.float64(F32(max_dist))


def sorted_neighbours(target, queries, kmax=KNN_MAX, chunk=256):
    """-> (d2 float64 [m, kmax], idx int64 [m, kmax]): per query the kmax smallest (d2, index) pairs over ALL target points, ascending
    (stable argsort); (inf, -1) beyond the target's size.  No cut-off yet: ``knn_from_sorted`` applies it."""
    T, Q = _clouds(target, queries)
    m, n = len(Q), len(T)
    d2s, idxs = np.full((m, kmax), np.inf), np.full((m, kmax), -1, np.int64)
    w = min(kmax, n)
    for s in range(0, m, chunk) if n else ():
        d2 = _d2(T, Q[s:s + chunk])
        order = np.argsort(d2, axis=1, kind="stable")[:, :w]
        d2s[s:s + chunk, :w] = np.take_along_axis(d2, order, 1)
        idxs[s:s + chunk, :w] = order
    return d2s, idxs


def knn_from_sorted(d2s, idxs, k, max_dist):
    """-> (dist float32 [m, k], idx int64 [m, k], count int32 [m], mean float64 [m]): the first k entries with d2 <= limit (inf is never
    within: the limit is finite); unused slots (inf, -1); mean = ((s_0 + s_1) + ...) / count with s_j = sqrt(d2_j), +inf for count 0"""
    d2, idx = d2s[:, :k], idxs[:, :k]
    used = np.isfinite(d2) & (d2 <= limit_of(max_dist))
    root = np.sqrt(np.where(used, d2, 0.0))
    dist = np.where(used, root.astype(F32), F32(np.inf)).astype(F32)
    count = used.sum(1).astype(np.int32)
    total = np.zeros(len(d2))
    for j in range(d2.shape[1]):                             # in ascending order, one addition at a time (the used slots are a prefix)
        total = np.where(used[:, j], total + root[:, j], total)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(count > 0, total / count, np.inf)
    return dist, np.where(used, idx, -1), count, mean


def knn(target, queries, k, max_dist):
    return knn_from_sorted(*sorted_neighbours(target, queries, k), k, max_dist)


def count_within(target, queries, radius, chunk=256):
    """int32 [m]: the number of target points with d2 <= double(float32(radius))^2"""
    T, Q = _clouds(target, queries)
    out = np.zeros(len(Q), np.int32)
    for s in range(0, len(Q), chunk) if len(T) else ():
        out[s:s + chunk] = (_d2(T, Q[s:s + chunk]) <= limit_of(radius)).sum(1)
    return out


def statistical_outliers(points, k, std_ratio, max_dist, sorted_pairs=None):
    """-> (kept indices int64 ascending, {"mean", "valid", "mu", "sigma", "threshold", "n_valid"}): the cloud on itself; valid iff k neighbours
    within max_dist; mu, sigma (n - 1) over the valid means; kept iff valid and mean < mu + std_ratio * sigma; fewer than 2 valid: all valid"""
    pairs = sorted_neighbours(points, points, k) if sorted_pairs is None else sorted_pairs
    _, _, count, mean = knn_from_sorted(*pairs, k, max_dist)
    valid = count == k
    info = {"mean": mean, "valid": valid, "mu": float("nan"), "sigma": float("nan"), "threshold": float("inf"), "n_valid": int(valid.sum())}
    keep = valid
    if info["n_valid"] >= 2:
        v = mean[valid]
        mu = float(v.sum() / len(v))
        sigma = float(np.sqrt(((v - mu) ** 2).sum() / (len(v) - 1)))
        info.update(mu=mu, sigma=sigma, threshold=mu + std_ratio * sigma)
        keep = valid & (mean < info["threshold"])
    return np.flatnonzero(keep).astype(np.int64), info


def radius_outliers(points, radius, min_neighbours):
    return np.flatnonzero(count_within(points, points, radius) > min_neighbours).astype(np.int64)


# ---------------------------------------------------------------- the makers of the test clouds
def cube(n, seed, lo=0.0, hi=1.0):
    return (lo + (hi - lo) * np.random.default_rng(seed).random((n, 3))).astype(F32)


def random_pair():
    """(5000 targets, 3000 queries) in the unit cube: uniform, but for 1000 targets and 300 queries inside the box [0.3, 0.38]^3"""
    t, q = cube(5000, 1), cube(3000, 2)
    t[4000:] = cube(1000, 3, 0.3, 0.38)
    q[2700:] = cube(300, 4, 0.3, 0.38)
    return t, q


def lattice():
    """the planar lattice k * float32(0.1), k = -20 .. 20, in x and y: index 41 i + j; every coordinate on (or an ulp beside) a cell face"""
    k = np.arange(-20, 21).astype(F32) * F32(0.1)
    x, y = np.meshgrid(k, k, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.zeros(x.size, F32)], 1).astype(F32)


FILTER_MAX_DIST = 0.06
FILTER_RADIUS = 0.03
FILTER_MIN_NEIGHBOURS = 5
FILTER_SEED = 41


def wavy_surface(seed=FILTER_SEED, n=4000, planted=40):
    """n points of the surface z = 0.05 sin(6 x) cos(5 y) over the unit square, then ``planted`` floaters: a 0.1-spaced grid at z >= 0.5 -
    farther than FILTER_MAX_DIST from one another and from the surface; shuffled.  -> (points float32 [n + planted, 3], the floaters' indices)"""
    g = np.random.default_rng(seed)
    xy = g.random((n, 2))
    surf = np.concatenate([xy, (0.05 * np.sin(6 * xy[:, :1]) * np.cos(5 * xy[:, 1:]))], 1)
    i = np.arange(planted)
    floaters = np.stack([0.1 * (i % 8) + 0.05, 0.1 * (i // 8) + 0.05, 0.5 + 0.1 * (i % 3)], 1)
    perm = g.permutation(n + planted)
    pts = np.concatenate([surf, floaters])[perm].astype(F32)
    return pts, np.sort(np.flatnonzero(perm >= n))
