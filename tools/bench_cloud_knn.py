"""k nearest neighbours and the outlier filters on a cloud the project itself produces: the default-form cloud of the synthetic
scan of tools/bench_cloud_eval.py, indexed on itself.

    python tools/bench_cloud_knn.py [--views 49] [--size 1184x1600] [--neighbours 10] [--rounds 3] [--out profiles/cloud_knn_bench.json]

max_dist = 1 % of the bounding-box diagonal, cell = max_dist / 4.  Between HIP events, medians of --rounds rounds after a warm-up: `knn` at
k = 1, 8, 20, 32 (query keys, sort and the kernel), `nearest` on the same inputs beside k = 1 (the difference is what the list costs),
`knn_mean_distance` at k = 20 (no [m, k] lists written), `count_within` at max_dist / 2.  Then the index build and `knn` at k = 20 with the
cell at max_dist / 1, 2, 4, 8 - what the filters' default cell rests on.  The comparator is scipy's
`cKDTree.query(k=20, distance_upper_bound=max_dist, workers=16)` on the host clock, interleaved with the device path round by round; its
neighbour lists are compared with the device's.  Last, both filters' kept counts and whole-call times.  Needs a GPU."""
import argparse
import json
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

KS = (1, 8, 20, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--size", default="1184x1600", help="HxW of the images")
    ap.add_argument("--neighbours", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=16, help="GRU iterations per cascade stage")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cloud_knn_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cloud_knn: needs a GPU")
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
    model = RAFT(cascade=cascade, test_mode=True)
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=5))
    model = model.to(dev).eval()
    one = [0] + pairs[0][:nb]
    with torch.no_grad():
        for _ in range(3):                                   # (the default form calibrates on its first forwards)
            model(images[one][None].to(dev), poses[one][None].to(dev), intr[one][None].to(dev), scale=scale)
    out = reconstruct_scan(model, images, poses, intr, names, pairs, scales, None, num_frames=nb, glb=0.25, streams=3, write=False)
    cloud = torch.from_numpy(np.ascontiguousarray(out["xyz"], np.float32)).to(dev)
    form = str(getattr(model, "auto_choice", None))
    del model
    torch.cuda.empty_cache()
    n = len(cloud)
    diag = float((cloud.amax(0) - cloud.amin(0)).double().norm())
    max_dist = float(np.float32(0.01 * diag))
    cell = max_dist / CE.DEFAULT_CELL_DIVISOR
    print(f"cloud: form {form}, {n} points, max_dist {max_dist:.6g}", flush=True)
    result = {"views": M, "height": H, "width": W, "neighbours": nb, "gru_iterations": 2 * args.iters, "rounds": args.rounds,
              "device": torch.cuda.get_device_name(0), "form": form, "points": n, "bbox_diagonal": diag, "max_dist": max_dist, "cell": cell}

    # ---- the searches, the device and the host interleaved
    c_np = cloud.cpu().numpy().astype(np.float64)
    index = CE.CloudIndex(cloud, cell)
    for k in KS:                                             # warm-up of every path
        index.knn(cloud, k, max_dist)
    index.nearest(cloud, max_dist)
    index.knn_mean_distance(cloud, 20, max_dist)
    index.count_within(cloud, max_dist / 2)
    torch.cuda.synchronize()
    rows = {f"knn_k{k}_ms": [] for k in KS}
    rows.update({"index_build_ms": [], "nearest_ms": [], "knn_mean_distance_k20_ms": [], "count_within_half_max_dist_ms": [], "kdtree_build_ms": [],
                 "kdtree_query_k20_ms": []})
    for _ in range(args.rounds):
        index, ms = timed(lambda: CE.CloudIndex(cloud, cell))
        rows["index_build_ms"].append(ms)
        for k in KS:
            got, ms = timed(lambda: index.knn(cloud, k, max_dist))
            rows[f"knn_k{k}_ms"].append(ms)
            if k == 20:
                d20, i20, c20 = got
        _, ms = timed(lambda: index.nearest(cloud, max_dist))
        rows["nearest_ms"].append(ms)
        _, ms = timed(lambda: index.knn_mean_distance(cloud, 20, max_dist))
        rows["knn_mean_distance_k20_ms"].append(ms)
        _, ms = timed(lambda: index.count_within(cloud, max_dist / 2))
        rows["count_within_half_max_dist_ms"].append(ms)
        t0 = time.perf_counter()
        tree = cKDTree(c_np)
        t1 = time.perf_counter()
        kd, ki = tree.query(c_np, k=20, distance_upper_bound=max_dist, workers=16)
        t2 = time.perf_counter()
        rows["kdtree_build_ms"].append(1e3 * (t1 - t0))
        rows["kdtree_query_k20_ms"].append(1e3 * (t2 - t1))
    med = {k: statistics.median(v) for k, v in rows.items()}
    d_np, c_dev = d20.cpu().numpy().astype(np.float64), c20.cpu().numpy()
    both = np.isfinite(kd) & np.isfinite(d_np)
    result["time"] = {"all_rounds": rows, **med, "index_cells": index.cells,
                      "list_cost_k1_over_nearest": med["knn_k1_ms"] / med["nearest_ms"],
                      "kdtree_query_over_knn_k20": med["kdtree_query_k20_ms"] / med["knn_k20_ms"],
                      "kdtree_total_over_hip_total_k20": (med["kdtree_build_ms"] + med["kdtree_query_k20_ms"]) / (med["index_build_ms"] + med["knn_k20_ms"]),
                      "full_rows_k20": int((c_dev == 20).sum()), "empty_rows_k20": int((c_dev == 0).sum()),
                      "counts_equal_kdtree": bool(np.array_equal(np.isfinite(kd).sum(1), c_dev)),
                      "max_abs_dist_difference_to_kdtree": float(np.abs(kd[both] - d_np[both]).max()) if both.any() else None}
    print(json.dumps({k: v for k, v in result["time"].items() if k != "all_rounds"}), flush=True)

    # ---- the cell at k = 20
    sweep = []
    for div in (1, 2, 4, 8):
        c = max_dist / div
        b, s = [], []
        for _ in range(args.rounds):
            ix, ms = timed(lambda: CE.CloudIndex(cloud, c))
            b.append(ms)
            _, ms = timed(lambda: ix.knn(cloud, 20, max_dist))
            s.append(ms)
        sweep.append({"divisor": div, "cell": c, "cells": ix.cells, "build_ms": statistics.median(b), "knn_k20_ms": statistics.median(s)})
    best = min(sweep, key=lambda r: r["build_ms"] + r["knn_k20_ms"])
    result["cell_sweep"] = sweep
    result["cell_sweep_best_divisor"] = best["divisor"]
    print(json.dumps(sweep), flush=True)

    # ---- the filters
    info_s, info_r = {}, {}
    keep_s, ms_s = timed(lambda: CE.remove_statistical_outliers(cloud, k=20, std_ratio=2.0, max_dist=max_dist, info=info_s))
    keep_r, ms_r = timed(lambda: CE.remove_radius_outliers(cloud, max_dist / 2, 8, info=info_r))
    result["filters"] = {"statistical": {**info_s, "ms": ms_s, "k": 20, "std_ratio": 2.0, "n_in": n},
                         "radius": {**info_r, "ms": ms_r, "min_neighbours": 8, "n_in": n}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"filters": result["filters"], "cell_sweep_best_divisor": best["divisor"], "out": args.out}))


if __name__ == "__main__":
    main()
