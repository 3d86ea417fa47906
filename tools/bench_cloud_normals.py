"""Surface normals on the cloud tools/bench_cloud_knn.py uses: the default-form cloud of the synthetic scan of
tools/bench_cloud_eval.py, indexed on itself.

    python tools/bench_cloud_normals.py [--views 49] [--size 1184x1600] [--neighbours 10] [--rounds 3] [--out profiles/cloud_normals_bench.json]

max_dist = 1 % of the bounding-box diagonal, cell = max_dist / 4.  Between HIP events, medians of --rounds rounds after a warm-up: `normals`
at k = 8, 20, 32 with and without viewpoints (query keys, sort and the kernel) beside `knn` at the same k on the same inputs - the difference
is what the epilogue costs (the gather of the neighbours' coordinates, nine fp64 sums, the Jacobi sweeps) minus the [m, k] lists `knn` writes
and `normals` does not.  The comparator is the host: scipy's `cKDTree.query(k=20, distance_upper_bound=max_dist, workers=16)` plus a batched
`numpy.linalg.eigh` of the covariances, on the host clock, interleaved with the device path round by round; its normals are compared with
the device's.  Last, `reconstruct_scan` with and without `normals=True`, whole calls on the host clock.  Needs a GPU."""
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

KS = (8, 20, 32)


def host_normals(tree, pts, k, max_dist):
    """the host path: neighbours from the k-d tree, covariances about the neighbourhood's mean, batched eigh -> (normal [n, 3], valid [n])"""
    d, i = tree.query(pts, k=k, distance_upper_bound=max_dist, workers=16)
    used = np.isfinite(d)
    c = used.sum(1)
    nb = np.where(used[:, :, None], pts[np.minimum(i, len(pts) - 1)] - pts[:, None, :], 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = nb.sum(1) / c[:, None]
        cov = np.einsum("nka,nkb->nab", nb, nb) / c[:, None, None] - mean[:, :, None] * mean[:, None, :]
    ok = c >= 3
    lam, vec = np.linalg.eigh(np.where(ok[:, None, None], cov, np.eye(3)))
    return vec[:, :, 0], ok & (lam[:, 2] > 0) & (lam[:, 1] > 1e-12 * lam[:, 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--size", default="1184x1600", help="HxW of the images")
    ap.add_argument("--neighbours", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=16, help="GRU iterations per cascade stage")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cloud_normals_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cloud_normals: needs a GPU")
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

    # ---- reconstruct_scan with and without normals, whole calls, interleaved (the first plain call is the warm-up and gives the cloud)
    scan = lambda **kw: reconstruct_scan(model, images, poses, intr, names, pairs, scales, None, num_frames=nb, glb=0.25, streams=3, write=False, **kw)
    out = scan()
    scan(normals=True)
    rows = {"reconstruct_scan_s": [], "reconstruct_scan_normals_s": []}
    for _ in range(args.rounds):
        for key, kw in (("reconstruct_scan_s", {}), ("reconstruct_scan_normals_s", {"normals": True})):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = scan(**kw)
            rows[key].append(time.perf_counter() - t0)
    scan_info = got["normal_info"]
    cloud = torch.from_numpy(np.ascontiguousarray(out["xyz"], np.float32)).to(dev)
    form = str(getattr(model, "auto_choice", None))
    del model, got
    torch.cuda.empty_cache()
    n = len(cloud)
    diag = float((cloud.amax(0) - cloud.amin(0)).double().norm())
    max_dist = float(np.float32(0.01 * diag))
    cell = max_dist / CE.KNN_CELL_DIVISOR
    print(f"cloud: form {form}, {n} points, max_dist {max_dist:.6g}", flush=True)
    result = {"views": M, "height": H, "width": W, "neighbours": nb, "gru_iterations": 2 * args.iters, "rounds": args.rounds,
              "device": torch.cuda.get_device_name(0), "form": form, "points": n, "bbox_diagonal": diag, "max_dist": max_dist, "cell": cell,
              "reconstruct_scan": {"all_rounds": rows, **{k: statistics.median(v) for k, v in rows.items()}, "normal_info": scan_info}}
    print(json.dumps({k: v for k, v in result["reconstruct_scan"].items() if k != "all_rounds"}), flush=True)

    # ---- the kernel beside knn, the device and the host interleaved
    c_np = cloud.cpu().numpy().astype(np.float64)
    centre = cloud.mean(0) + torch.tensor([0.0, 0.0, diag], device=dev)      # one viewpoint off the cloud; a [n, 3] tensor as the scan passes it
    vps = centre[None].expand(n, 3).contiguous()
    index = CE.CloudIndex(cloud, cell)
    for k in KS:                                             # warm-up of every path
        index.knn(cloud, k, max_dist)
        index.normals(cloud, k, max_dist)
        index.normals(cloud, k, max_dist, viewpoints=vps)
    torch.cuda.synchronize()
    rows = {f"{what}_k{k}_ms": [] for k in KS for what in ("knn", "normals", "normals_viewpoints")}
    rows.update({"kdtree_build_ms": [], "host_normals_k20_ms": []})
    for _ in range(args.rounds):
        for k in KS:
            _, ms = timed(lambda: index.knn(cloud, k, max_dist))
            rows[f"knn_k{k}_ms"].append(ms)
            got, ms = timed(lambda: index.normals(cloud, k, max_dist))
            rows[f"normals_k{k}_ms"].append(ms)
            if k == 20:
                n20, c20, cnt20 = got
            _, ms = timed(lambda: index.normals(cloud, k, max_dist, viewpoints=vps))
            rows[f"normals_viewpoints_k{k}_ms"].append(ms)
        t0 = time.perf_counter()
        tree = cKDTree(c_np)
        t1 = time.perf_counter()
        hn, hv = host_normals(tree, c_np, 20, max_dist)
        t2 = time.perf_counter()
        rows["kdtree_build_ms"].append(1e3 * (t1 - t0))
        rows["host_normals_k20_ms"].append(1e3 * (t2 - t1))
    med = {k: statistics.median(v) for k, v in rows.items()}
    dn = n20.cpu().numpy().astype(np.float64)
    dv = ~np.isnan(c20.cpu().numpy())
    both = dv & hv
    cos = np.abs((dn[both] * hn[both]).sum(1))
    result["time"] = {"all_rounds": rows, **med,
                      **{f"epilogue_over_knn_k{k}": med[f"normals_k{k}_ms"] / med[f"knn_k{k}_ms"] for k in KS},
                      "host_over_normals_k20": med["host_normals_k20_ms"] / med["normals_k20_ms"],
                      "valid_k20": int(dv.sum()), "valid_equal_host": bool(np.array_equal(dv, hv)),
                      "full_rows_k20": int((cnt20.cpu().numpy() == 20).sum()),
                      "max_angle_to_host_degrees": float(np.degrees(np.arccos(np.clip(cos.min(), -1, 1)))) if both.any() else None,
                      "median_angle_to_host_degrees": float(np.degrees(np.arccos(np.clip(np.median(cos), -1, 1)))) if both.any() else None}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({**{k: v for k, v in result["time"].items() if k != "all_rounds"}, "out": args.out}))


if __name__ == "__main__":
    main()
