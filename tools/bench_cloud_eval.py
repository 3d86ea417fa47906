"""Cloud-to-cloud evaluation on the clouds the project itself produces: the synthetic scan of tools/bench_reconstruct.py goes through
`reconstruct_scan` twice - with gru_precision="s16" and with the default arithmetic form - and the two clouds are compared.

    python tools/bench_cloud_eval.py [--views 49] [--size 1184x1600] [--neighbours 10] [--rounds 3] [--out profiles/cloud_eval_bench.json]

First half, time.  Queries: the s16 cloud; target: the default form's cloud; max_dist = 1 % of the target's bounding-box diagonal.  Per round, one
after the other on the same box: (1) the HIP path - index build (keys, sort, cell table, record gather) and search (query keys, sort, kernel), each
between HIP events; (2) a chunked brute force in torch on the device (torch.cdist + min, float32) on the first 16 384 queries against the whole
target, between events, EXTRAPOLATED linearly to all queries; (3) scipy's cKDTree on the host (build, then query(distance_upper_bound=max_dist,
workers=16)), host clock.  Medians over the rounds.  Then the search at cell = max_dist / 1, 2, 4, 8 (what cloud_distances' default rests on).
Second half, what the arithmetic forms do to the product: accuracy / completeness / F between the two clouds beside the relative L1 of one
view's disparity maps.  Needs a GPU."""
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

from bench_scan import ring_pairs  # noqa: E402

SUBSET = 16384


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def brute_force(queries, target, chunk=1024):
    out = torch.empty(len(queries), device=queries.device)
    for s in range(0, len(queries), chunk):
        out[s:s + chunk] = torch.cdist(queries[s:s + chunk], target).min(1).values
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--size", default="1184x1600", help="HxW of the images")
    ap.add_argument("--neighbours", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=16, help="GRU iterations per cascade stage")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cloud_eval_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cloud_eval: needs a GPU")
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

    clouds, disps, forms = {}, {}, {}
    one = [0] + pairs[0][:nb]
    for name, kw in (("s16", {"gru_precision": "s16"}), ("default", {})):
        model = RAFT(cascade=cascade, test_mode=True, **kw)
        model.load_state_dict(fill_state_dict(model.state_dict(), seed=5))
        model = model.to(dev).eval()
        with torch.no_grad():
            for _ in range(3):                               # (the default form calibrates on its first forwards)
                d = model(images[one][None].to(dev), poses[one][None].to(dev), intr[one][None].to(dev), scale=scale)
        disps[name] = d.double().cpu()
        out = reconstruct_scan(model, images, poses, intr, names, pairs, scales, None, num_frames=nb, glb=0.25, streams=3, write=False)
        clouds[name] = torch.from_numpy(np.ascontiguousarray(out["xyz"], np.float32)).to(dev)
        forms[name] = str(getattr(model, "auto_choice", None) or kw.get("gru_precision"))
        print(f"{name}: form {forms[name]}, {len(out['xyz'])} points", flush=True)
        del model
    torch.cuda.empty_cache()
    queries, target = clouds["s16"], clouds["default"]
    lo, hi = target.amin(0), target.amax(0)
    diag = float((hi - lo).double().norm())
    max_dist = float(np.float32(0.01 * diag))
    tau = max_dist / 4
    result = {"views": M, "height": H, "width": W, "neighbours": nb, "gru_iterations": 2 * args.iters, "rounds": args.rounds,
              "device": torch.cuda.get_device_name(0), "forms": forms, "queries": len(queries), "target": len(target), "bbox_diagonal": diag,
              "max_dist": max_dist, "tau": tau, "default_cell": max_dist / CE.DEFAULT_CELL_DIVISOR}

    # ---- first half: time
    cell = max_dist / CE.DEFAULT_CELL_DIVISOR
    q_np, t_np = queries.cpu().numpy().astype(np.float64), target.cpu().numpy().astype(np.float64)
    sub = queries[:SUBSET].contiguous()
    index = CE.CloudIndex(target, cell)                      # warm-up of every path
    dist, idx = index.nearest(queries, max_dist)
    brute_force(sub[:2048], target)
    torch.cuda.synchronize()
    rows = {"hip_build_ms": [], "hip_search_ms": [], "brute_subset_ms": [], "kdtree_build_ms": [], "kdtree_query_ms": []}
    for _ in range(args.rounds):
        index, ms = timed(lambda: CE.CloudIndex(target, cell))
        rows["hip_build_ms"].append(ms)
        (dist, idx), ms = timed(lambda: index.nearest(queries, max_dist))
        rows["hip_search_ms"].append(ms)
        bf, ms = timed(lambda: brute_force(sub, target))
        rows["brute_subset_ms"].append(ms)
        t0 = time.perf_counter()
        tree = cKDTree(t_np)
        t1 = time.perf_counter()
        kd, ki = tree.query(q_np, distance_upper_bound=max_dist, workers=16)
        t2 = time.perf_counter()
        rows["kdtree_build_ms"].append(1e3 * (t1 - t0))
        rows["kdtree_query_ms"].append(1e3 * (t2 - t1))
    med = {k: statistics.median(v) for k, v in rows.items()}
    hip_all = med["hip_build_ms"] + med["hip_search_ms"]
    brute_all = med["brute_subset_ms"] * len(queries) / len(sub)
    kd_all = med["kdtree_build_ms"] + med["kdtree_query_ms"]
    d_np = dist.cpu().numpy().astype(np.float64)
    both = np.isfinite(kd) & np.isfinite(d_np)
    result["time"] = {"cell": cell, "index_cells": index.cells, "all_rounds": rows, **med,
                      "hip_total_ms": hip_all,
                      "brute_force_total_ms_extrapolated": brute_all, "brute_force_subset": len(sub),
                      "kdtree_total_ms": kd_all,
                      "brute_force_over_hip_search": brute_all / med["hip_search_ms"], "brute_force_over_hip_total": brute_all / hip_all,
                      "kdtree_query_over_hip_search": med["kdtree_query_ms"] / med["hip_search_ms"], "kdtree_total_over_hip_total": kd_all / hip_all,
                      "hip_is_faster_than_both": bool(hip_all < brute_all and hip_all < kd_all),
                      "found_hip": int(np.isfinite(d_np).sum()), "found_kdtree": int(np.isfinite(kd).sum()),
                      "max_abs_dist_difference_to_kdtree": float(np.abs(kd[both] - d_np[both]).max()) if both.any() else None,
                      "max_abs_dist_difference_to_brute_force_f32": float((bf - dist[:len(sub)]).abs()[torch.isfinite(dist[:len(sub)])].max())}
    print(json.dumps({k: v for k, v in result["time"].items() if k != "all_rounds"}), flush=True)
    sweep = []
    for div in (1, 2, 4, 8):
        c = max_dist / div
        b, s = [], []
        for _ in range(args.rounds):
            ix, ms = timed(lambda: CE.CloudIndex(target, c))
            b.append(ms)
            _, ms = timed(lambda: ix.nearest(queries, max_dist))
            s.append(ms)
        sweep.append({"divisor": div, "cell": c, "cells": ix.cells, "build_ms": statistics.median(b), "search_ms": statistics.median(s)})
    result["cell_sweep"] = sweep
    print(json.dumps(sweep), flush=True)

    # ---- second half: the two forms' clouds
    result["clouds"] = {"dtu": CE.accuracy_completeness(queries, target, max_dist=max_dist),
                        "fscore": CE.fscore(queries, target, tau),
                        "fscore_at_max_dist_over_40": CE.fscore(queries, target, max_dist / 40),
                        "disparity_rel_l1_view0": float((disps["s16"] - disps["default"]).abs().sum() / disps["default"].abs().sum())}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"clouds": result["clouds"], "out": args.out}))


if __name__ == "__main__":
    main()
