"""A numpy fp64 restatement of the surface normals of cer-mvs_amd/cloud_eval.py (csrc/cloud_eval.hip grid_normals_kernel),
shared by test_cloud_normals_cpu.py and test_cloud_normals_gpu.py.  Written from the contract, importing nothing from the package: the
neighbour lists are knn_reference's (``sorted_neighbours`` / ``knn_from_sorted``); the nine sums about the query run as a loop over the k
slots in ascending order, vectorised over the queries, one addition at a time; then C = S2 / c - mean mean^T, ``numpy.linalg.eigh``, the
validity rule, the canonical sign and the viewpoint flip."""
import numpy as np

import knn_reference as R

F32 = np.float32
NORMAL_DEGENERATE = 1e-12
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))   # S2's order: xx xy xz yy yz zz


def moments(target, queries, idx):
    """-> float64 [m, 9]: S1 (3) then S2 (6) of d_j = double(p_j) - double(q) over the used slots of ``idx`` ([m, k], -1: unused), added in
    slot order; zeros for a row without a used slot"""
    T, Q = np.asarray(target, F32).astype(np.float64).reshape(-1, 3), np.asarray(queries, F32).astype(np.float64).reshape(-1, 3)
    m = len(Q)
    mom = np.zeros((m, 9))
    for j in range(idx.shape[1]):
        used = idx[:, j] >= 0
        with np.errstate(invalid="ignore", over="ignore"):
            d = T[np.maximum(idx[:, j], 0)] - Q if len(T) else np.zeros((m, 3))
            terms = [d[:, 0], d[:, 1], d[:, 2]] + [d[:, a] * d[:, b] for a, b in PAIRS]
            for s, term in enumerate(terms):
                mom[:, s] = np.where(used, mom[:, s] + term, mom[:, s])
    return mom


def covariance(mom, count):
    """-> float64 [m, 3, 3]: C_ab = S2_ab / c - (S1_a / c) * (S1_b / c); NaN rows where c = 0"""
    c = np.asarray(count, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = mom[:, :3] / c[:, None]
        C = np.empty((len(c), 3, 3))
        for s, (a, b) in enumerate(PAIRS):
            C[:, a, b] = C[:, b, a] = mom[:, 3 + s] / c - mean[:, a] * mean[:, b]
    return C


def canonical(n):
    """the component of largest magnitude positive, the lowest axis on a tie (np.argmax takes the first maximum)"""
    lead = np.take_along_axis(n, np.argmax(np.abs(n), axis=1)[:, None], 1)
    return np.where(lead < 0, -n, n)


def normals_from_lists(target, queries, idx, count, viewpoints=None):
    """-> dict: "normal" float32 [m, 3], "curvature" float32 [m], "valid" bool [m], "mom" float64 [m, 9], "lam" float64 [m, 3] (ascending; NaN
    where count = 0 or the query is not finite), "n64" the fp64 normal in its final sign, "s" the viewpoint test's fp64 dot product (with
    the canonical normal) and "vnorm" the length of viewpoint - query (both NaN without viewpoints)"""
    Q = np.asarray(queries, F32).astype(np.float64).reshape(-1, 3)
    m = len(Q)
    mom = moments(target, queries, idx)
    C = covariance(mom, count)
    finite = np.isfinite(Q).all(1)
    ok = finite & (count >= 1) & np.isfinite(C).all((1, 2))
    lam, vec = np.full((m, 3), np.nan), np.zeros((m, 3, 3))
    if ok.any():
        lam[ok], vec[ok] = np.linalg.eigh(C[ok])
    with np.errstate(invalid="ignore"):
        valid = ok & (count >= 3) & (lam[:, 2] > 0) & (lam[:, 1] > NORMAL_DEGENERATE * lam[:, 2])
        curv = np.maximum(lam[:, 0], 0.0) / ((lam[:, 0] + lam[:, 1]) + lam[:, 2])
    n = canonical(vec[:, :, 0])
    s, vnorm = np.full(m, np.nan), np.full(m, np.nan)
    if viewpoints is not None:
        V = np.broadcast_to(np.asarray(viewpoints, F32).astype(np.float64).reshape(-1, 3), (m, 3))
        with np.errstate(invalid="ignore", over="ignore"):
            v = V - Q
            s = (n[:, 0] * v[:, 0] + n[:, 1] * v[:, 1]) + n[:, 2] * v[:, 2]
            vnorm = np.sqrt((v * v).sum(1))
            flip = np.isfinite(V).all(1) & (s < 0)
        n = np.where(flip[:, None], -n, n)
    return {"normal": np.where(valid[:, None], n, 0.0).astype(F32), "curvature": np.where(valid, curv, np.nan).astype(F32), "valid": valid,
            "mom": mom, "lam": lam, "n64": n, "s": s, "vnorm": vnorm}


def normals(target, queries, k, max_dist, viewpoints=None, sorted_pairs=None):
    """the whole estimate: knn_reference's lists at (k, max_dist), then the above; "count" is added to the dict"""
    pairs = R.sorted_neighbours(target, queries, k) if sorted_pairs is None else (sorted_pairs[0][:, :k], sorted_pairs[1][:, :k])
    _, idx, count, _ = R.knn_from_sorted(*pairs, k, max_dist)
    out = normals_from_lists(target, queries, idx, count, viewpoints)
    out["count"] = count
    return out


def wavy_normal(xy):
    """the unit normal (n_z > 0) of z = 0.05 sin(6 x) cos(5 y), knn_reference.wavy_surface's surface, at ``xy`` [n, 2] (fp64)"""
    x, y = np.asarray(xy, np.float64)[:, 0], np.asarray(xy, np.float64)[:, 1]
    g = np.stack([-0.3 * np.cos(6 * x) * np.cos(5 * y), 0.25 * np.sin(6 * x) * np.sin(5 * y), np.ones_like(x)], 1)
    return g / np.linalg.norm(g, axis=1, keepdims=True)
