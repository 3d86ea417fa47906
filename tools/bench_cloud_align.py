"""Rigid registration (cloud_eval.icp) on the clouds the project itself produces: the synthetic scan of tools/bench_cloud_eval.py goes
through `reconstruct_scan` with gru_precision="s16" (the predicted cloud) and in the default arithmetic form (the ground truth); the predicted
cloud is moved by a planted rigid motion and registered back.

    python tools/bench_cloud_align.py [--views 49] [--size 1184x1600] [--rounds 3] [--angle 0.3] [--shift 0.3] [--out profiles/cloud_align_bench.json]

max_dist = 1 % of the ground truth's bounding-box diagonal (bench_cloud_eval's cut-off).  The planted motion: --angle degrees about (1, 2, 3)
through the cloud's centroid plus --shift x max_dist along (1, -1, 0.5).  Per round, one after the other on the same box: (1) `icp` as a whole,
host clock around it (it ends in a host read), and the index build between HIP events; (2) the same loop written out here with HIP events
around the transform, the query keys + sort, the search and the moments, and the host clock around the read of the 17 sums and the solve - its T
is checked against icp's, bit for bit; (3) the same loop on the host: scipy's cKDTree on the ground truth (built once, timed apart),
query(distance_upper_bound=max_dist, workers=16), numpy fp64 transform, moments and the same solve.  Medians over the rounds.  Recovery: the
largest |T P p - p| over the predicted cloud's points p (P the planted motion), for both.  Needs a GPU."""
import argparse
import json
import math
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_cloud_eval import timed  # noqa: E402
from bench_scan import ring_pairs  # noqa: E402

PARTS = ("transform_ms", "query_keys_sort_ms", "search_ms", "moments_ms", "host_read_solve_ms")


def planted_motion(centre, degrees, shift):
    u = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    th = math.radians(degrees)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)
    T[:3, 3] = centre - T[:3, :3] @ centre + shift * np.array([1.0, -1.0, 0.5]) / 1.5
    return T


def instrumented(CE, src, index, max_dist, max_iter=50, tol=1e-6):
    """cloud_eval.icp's loop with events around its parts -> (T, iterations, {part: [ms per iteration]})"""
    from cer_mvs_amd import _lib as L
    lib, dev, m = L.load(), src.device, len(src)
    pivot = np.array([float(v) for v in index.origin])
    T, prev, marks, host = np.eye(4), None, [], []

    def mark():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append(e)
    for it in range(max_iter):
        mark()
        cur = CE.rigid_transform(src, T)
        mark()
        qkeys = torch.empty(m, device=dev, dtype=torch.int64)
        L.check(lib.cer_grid_keys_f32(L.dev_ptr(cur, "queries"), m, index.origin, index.cell, 1, L.dev_ptr(qkeys, "keys", torch.int64), None,
                                      L.cur_stream()), "grid_keys")
        qorder = torch.sort(qkeys, stable=True).indices
        mark()
        idx = torch.empty(m, device=dev, dtype=torch.int64)
        dist = torch.empty(m, device=dev, dtype=torch.float32)
        L.check(lib.cer_grid_nearest_f32(*index.grid_args(), L.dev_ptr(cur, "queries"), L.dev_ptr(qorder, "qorder", torch.int64), m, max_dist,
                                         L.dev_ptr(idx, "idx", torch.int64), L.dev_ptr(dist, "dist"), L.cur_stream()), "grid_nearest")
        mark()
        partials = torch.empty(CE.MOMENT_COUNT * int(lib.cer_cloud_moment_partials(m)), device=dev, dtype=torch.float64)
        out = torch.empty(CE.MOMENT_COUNT, device=dev, dtype=torch.float64)
        L.check(lib.cer_cloud_pair_moments_f64(L.dev_ptr(cur, "a"), L.dev_ptr(index.points, "b"), L.dev_ptr(idx, "idx", torch.int64), m,
                                               (L._D * 3)(*pivot), L.dev_ptr(partials, "partials", torch.float64),
                                               L.dev_ptr(out, "out", torch.float64), L.cur_stream()), "cloud_pair_moments")
        mark()
        torch.cuda.synchronize()                             # (the device's share ends here; the copy below finds the sums ready)
        t0 = time.perf_counter()
        mom = out.cpu().numpy()
        k = int(mom[0])
        state = (k / m, math.sqrt(mom[16] / k) if k else 0.0)
        done = k < 3 or (prev is not None and abs(state[0] - prev[0]) < tol and abs(state[1] - prev[1]) < tol)
        if not done:
            T = CE.rigid_from_moments(mom, pivot) @ T
        host.append(1e3 * (time.perf_counter() - t0))
        prev = state
        if done:
            break
    ms = {p: [] for p in PARTS}
    for i in range(len(host)):
        e = marks[5 * i:5 * i + 5]
        for p, a, b in zip(PARTS, e, e[1:]):
            ms[p].append(a.elapsed_time(b))
        ms["host_read_solve_ms"].append(host[i])
    return T, len(host), ms


def host_icp(CE, tree, src64, dst64, max_dist, pivot, max_iter=50, tol=1e-6):
    """the loop on the host: fp64 transform rounded to float32, kd-tree query, numpy fp64 sums, the same solve -> (T, iterations, s per part)"""
    T, prev, n = np.eye(4), None, len(src64)
    parts = {"transform_s": 0.0, "query_s": 0.0, "moments_s": 0.0, "solve_s": 0.0}
    for it in range(max_iter):
        t0 = time.perf_counter()
        cur = (src64 @ T[:3, :3].T + T[:3, 3]).astype(np.float32).astype(np.float64)
        t1 = time.perf_counter()
        d, j = tree.query(cur, distance_upper_bound=max_dist, workers=16)
        t2 = time.perf_counter()
        ok = np.isfinite(d)
        A, B = cur[ok] - pivot, dst64[j[ok]] - pivot
        mom = np.concatenate([[float(ok.sum())], A.sum(0), B.sum(0), (A.T @ B).reshape(-1), [float((d[ok] * d[ok]).sum())]])
        t3 = time.perf_counter()
        k = int(mom[0])
        state = (k / n, math.sqrt(mom[16] / k) if k else 0.0)
        done = k < 3 or (prev is not None and abs(state[0] - prev[0]) < tol and abs(state[1] - prev[1]) < tol)
        if not done:
            T = CE.rigid_from_moments(mom, pivot) @ T
        t4 = time.perf_counter()
        for key, dt in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            parts[key] += dt
        prev = state
        if done:
            break
    return T, it + 1, parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--size", default="1184x1600", help="HxW of the images")
    ap.add_argument("--neighbours", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=16, help="GRU iterations per cascade stage")
    ap.add_argument("--angle", type=float, default=0.3, help="degrees of the planted rotation")
    ap.add_argument("--shift", type=float, default=0.3, help="planted translation, in units of max_dist")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cloud_align_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cloud_align: needs a GPU")
    dev = torch.device("cuda:0")
    from scipy.spatial import cKDTree
    from cer_mvs_amd import RAFT
    from cer_mvs_amd import cloud_eval as CE
    from cer_mvs_amd.scan import reconstruct_scan
    from cer_mvs_amd.synthetic import fill_state_dict, synthetic_scene

    H, W = (int(v) for v in args.size.lower().split("x"))
    M, nb = args.views, args.neighbours
    cascade = [(64, 64, args.iters), (-1, 320, args.iters)]
    t0 = time.perf_counter()
    images, poses, intr, scale = synthetic_scene(H, W, M - 1, seed=0)
    images, poses, intr = images[0].contiguous(), poses[0], intr[0]
    print(f"scene: {M} views of {W}x{H} in {time.perf_counter() - t0:.1f} s", flush=True)
    names, pairs, scales = [f"{i:08d}" for i in range(M)], ring_pairs(M, nb), [scale] * M
    clouds, forms = {}, {}
    one = [0] + pairs[0][:nb]
    for name, kw in (("s16", {"gru_precision": "s16"}), ("default", {})):
        model = RAFT(cascade=cascade, test_mode=True, **kw)
        model.load_state_dict(fill_state_dict(model.state_dict(), seed=5))
        model = model.to(dev).eval()
        with torch.no_grad():
            for _ in range(3):                               # (the default form calibrates on its first forwards)
                model(images[one][None].to(dev), poses[one][None].to(dev), intr[one][None].to(dev), scale=scale)
        out = reconstruct_scan(model, images, poses, intr, names, pairs, scales, None, num_frames=nb, glb=0.25, streams=3, write=False)
        clouds[name] = torch.from_numpy(np.ascontiguousarray(out["xyz"], np.float32)).to(dev)
        forms[name] = str(getattr(model, "auto_choice", None) or kw.get("gru_precision"))
        print(f"{name}: form {forms[name]}, {len(out['xyz'])} points", flush=True)
        del model
    torch.cuda.empty_cache()
    pred, dst = clouds["s16"], clouds["default"]
    diag = float((dst.amax(0) - dst.amin(0)).double().norm())
    max_dist = float(np.float32(0.01 * diag))
    pred64 = pred.double().cpu().numpy()
    planted = planted_motion(pred64.mean(0), args.angle, args.shift * max_dist)
    src = CE.rigid_transform(pred, planted)
    src64, dst64 = src.double().cpu().numpy(), dst.double().cpu().numpy()
    moved = float(np.abs(src64 - pred64).max())

    def recovery(T):                                         # largest |T P p - p| over the predicted cloud
        TP = T @ planted
        return float(np.abs(pred64 @ TP[:3, :3].T + TP[:3, 3] - pred64).max())
    cell = max_dist / CE.DEFAULT_CELL_DIVISOR
    result = {"views": M, "height": H, "width": W, "neighbours": nb, "gru_iterations": 2 * args.iters, "rounds": args.rounds,
              "device": torch.cuda.get_device_name(0), "forms": forms, "src": len(src), "dst": len(dst), "bbox_diagonal": diag, "max_dist": max_dist,
              "cell": cell, "planted": {"angle_degrees": args.angle, "shift": args.shift * max_dist, "largest_coordinate_move": moved,
                                        "T": planted.tolist()}}
    before = CE.fscore(src, dst, max_dist / 4)
    index = CE.CloudIndex(dst, cell)                         # warm-up of every path
    ref = CE.icp(src, dst, max_dist, index=index)
    instrumented(CE, src, index, max_dist, max_iter=2)
    torch.cuda.synchronize()
    rows = {"icp_total_ms": [], "index_build_ms": [], "instrumented_total_ms": [], "host_total_ms": [], "kdtree_build_ms": []}
    per_part, host_parts, host_T, host_iters = [], [], None, 0
    for _ in range(args.rounds):
        index, ms = timed(lambda: CE.CloudIndex(dst, cell))
        rows["index_build_ms"].append(ms)
        t0 = time.perf_counter()
        got = CE.icp(src, dst, max_dist, index=index)
        rows["icp_total_ms"].append(1e3 * (time.perf_counter() - t0))
        assert np.array_equal(got["T"], ref["T"]) and got["history"] == ref["history"]
        t0 = time.perf_counter()
        T, iters, ms = instrumented(CE, src, index, max_dist)
        torch.cuda.synchronize()
        rows["instrumented_total_ms"].append(1e3 * (time.perf_counter() - t0))
        assert np.array_equal(T, ref["T"]) and iters == ref["iterations"]
        per_part.append({p: statistics.median(v) for p, v in ms.items()})
        t0 = time.perf_counter()
        tree = cKDTree(dst64)
        rows["kdtree_build_ms"].append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        host_T, host_iters, parts = host_icp(CE, tree, src64, dst64, max_dist, np.array([float(v) for v in index.origin]))
        rows["host_total_ms"].append(1e3 * (time.perf_counter() - t0))
        host_parts.append({k[:-2] + "_ms": 1e3 * v / host_iters for k, v in parts.items()})
    med = {k: statistics.median(v) for k, v in rows.items()}
    part = {p: statistics.median(r[p] for r in per_part) for p in PARTS}
    after = CE.fscore(src, dst, max_dist / 4, align=ref["T"])
    result["device"] = {"name": result["device"], "iterations": ref["iterations"], "converged": ref["converged"], "fitness": ref["fitness"],
                        "rmse": ref["rmse"], "history": ref["history"], "T": ref["T"].tolist(), "all_rounds": rows, **med,
                        "icp_ms_per_iteration": med["icp_total_ms"] / ref["iterations"],
                        "per_iteration_median_ms": part, "per_iteration_sum_of_parts_ms": sum(part.values()),
                        "recovery_error": recovery(ref["T"]), "recovery_error_over_max_dist": recovery(ref["T"]) / max_dist}
    result["host"] = {"iterations": host_iters, "threads": 16, "total_ms": med["host_total_ms"], "kdtree_build_ms": med["kdtree_build_ms"],
                      "ms_per_iteration": med["host_total_ms"] / host_iters,
                      "per_iteration_ms": {k: statistics.median(r[k] for r in host_parts) for k in host_parts[0]},
                      "recovery_error": recovery(host_T), "T_difference_to_device": float(np.abs(host_T - ref["T"]).max())}
    result["host_over_device_per_iteration"] = result["host"]["ms_per_iteration"] / result["device"]["icp_ms_per_iteration"]
    result["fscore_at_max_dist_over_4"] = {"moved": before, "registered": after, "unmoved": CE.fscore(pred, dst, max_dist / 4)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in result["device"].items() if k not in ("all_rounds", "history", "T")}))
    print(json.dumps(result["host"]))
    print(json.dumps({"host_over_device_per_iteration": result["host_over_device_per_iteration"], "out": args.out}))


if __name__ == "__main__":
    main()
