"""Point-to-plane against point-to-point ICP (cloud_eval.icp(method="plane")) on the clouds tools/bench_cloud_align.py builds: the
synthetic scan through `reconstruct_scan` with gru_precision="s16" (the predicted cloud) and in the default arithmetic form (the ground
truth), the predicted cloud moved by the same planted rigid motion and registered back.

    python tools/bench_cloud_align_plane.py [--views 49] [--size 1184x1600] [--rounds 3] [--angle 0.3] [--shift 0.3] [--normals-k 20]
                                            [--out profiles/cloud_align_plane_bench.json]

max_dist, the cell and the planted motion are bench_cloud_align's.  The ground truth's normals are estimated once (`estimate_normals`, k =
--normals-k; timed between HIP events, per round) and handed to every plane run.  Per round, one after the other on the same box, the index
built once and shared: `icp(method="point")`, then `icp(method="plane")`, host clock around each (both end in a host read); then, on the
matches of the first iteration, `pair_moments`' and `plane_moments`' entry points between HIP events.  Medians over the rounds.  Recovery: the
largest |T P p - p| over the predicted cloud's points p (P the planted motion).  Needs a GPU."""
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

from bench_cloud_align import planted_motion  # noqa: E402
from bench_cloud_eval import timed  # noqa: E402
from bench_scan import ring_pairs  # noqa: E402


def build_clouds(args, dev):
    """(predicted, ground truth, forms): bench_cloud_align's two reconstructions of its synthetic scan"""
    from cer_mvs_amd import RAFT
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
    return clouds["s16"], clouds["default"], forms


def moment_kernels(CE, cur, index, nrm, idx):
    """(pair_moments ms, plane_moments ms) of the two entry points on the same pairs, between events; buffers allocated outside"""
    from cer_mvs_amd import _lib as L
    lib, dev, m = L.load(), cur.device, len(cur)
    pivot = (L._D * 3)(*[float(v) for v in index.origin])
    np_ = int(lib.cer_cloud_moment_partials(m))
    buf = {n: (torch.empty(n * np_, device=dev, dtype=torch.float64), torch.empty(n, device=dev, dtype=torch.float64))
           for n in (CE.MOMENT_COUNT, CE.PLANE_MOMENT_COUNT)}
    a, b, pi = L.dev_ptr(cur, "a"), L.dev_ptr(index.points, "b"), L.dev_ptr(idx, "idx", torch.int64)

    def pair():
        part, out = buf[CE.MOMENT_COUNT]
        L.check(lib.cer_cloud_pair_moments_f64(a, b, pi, m, pivot, L.dev_ptr(part, "partials", torch.float64), L.dev_ptr(out, "out", torch.float64),
                                               L.cur_stream()), "cloud_pair_moments")

    def plane():
        part, out = buf[CE.PLANE_MOMENT_COUNT]
        L.check(lib.cer_cloud_plane_moments_f64(a, b, L.dev_ptr(nrm, "normals"), pi, m, pivot, L.dev_ptr(part, "partials", torch.float64),
                                                L.dev_ptr(out, "out", torch.float64), L.cur_stream()), "cloud_plane_moments")
    return timed(pair)[1], timed(plane)[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--size", default="1184x1600", help="HxW of the images")
    ap.add_argument("--neighbours", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=16, help="GRU iterations per cascade stage")
    ap.add_argument("--angle", type=float, default=0.3, help="degrees of the planted rotation")
    ap.add_argument("--shift", type=float, default=0.3, help="planted translation, in units of max_dist")
    ap.add_argument("--normals-k", type=int, default=20, help="neighbours behind the ground truth's normals")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cloud_align_plane_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cloud_align_plane: needs a GPU")
    dev = torch.device("cuda:0")
    from cer_mvs_amd import cloud_eval as CE

    pred, dst, forms = build_clouds(args, dev)
    diag = float((dst.amax(0) - dst.amin(0)).double().norm())
    max_dist = float(np.float32(0.01 * diag))
    pred64 = pred.double().cpu().numpy()
    planted = planted_motion(pred64.mean(0), args.angle, args.shift * max_dist)
    src = CE.rigid_transform(pred, planted)

    def recovery(T):                                         # largest |T P p - p| over the predicted cloud
        TP = T @ planted
        return float(np.abs(pred64 @ TP[:3, :3].T + TP[:3, 3] - pred64).max())
    cell = max_dist / CE.DEFAULT_CELL_DIVISOR
    index = CE.CloudIndex(dst, cell)                         # warm-up of every path
    info = {}
    nrm = CE.estimate_normals(dst, k=args.normals_k, info=info)[0]
    ref = {"point": CE.icp(src, dst, max_dist, index=index), "plane": CE.icp(src, dst, max_dist, index=index, method="plane", dst_normals=nrm)}
    first = index.nearest(src, max_dist)[1]
    moment_kernels(CE, src, index, nrm, first)
    torch.cuda.synchronize()
    rows = {"point_total_ms": [], "plane_total_ms": [], "normals_ms": [], "pair_moments_ms": [], "plane_moments_ms": []}
    for _ in range(args.rounds):
        for name, kw in (("point", {}), ("plane", {"method": "plane", "dst_normals": nrm})):
            t0 = time.perf_counter()
            got = CE.icp(src, dst, max_dist, index=index, **kw)
            rows[name + "_total_ms"].append(1e3 * (time.perf_counter() - t0))
            assert np.array_equal(got["T"], ref[name]["T"]) and got["history"] == ref[name]["history"]
        rows["normals_ms"].append(timed(lambda: CE.estimate_normals(dst, k=args.normals_k))[1])
        pair_ms, plane_ms = moment_kernels(CE, src, index, nrm, first)
        rows["pair_moments_ms"].append(pair_ms)
        rows["plane_moments_ms"].append(plane_ms)
    med = {k: statistics.median(v) for k, v in rows.items()}
    result = {"views": args.views, "size": args.size, "neighbours": args.neighbours, "gru_iterations": 2 * args.iters, "rounds": args.rounds,
              "device": torch.cuda.get_device_name(0), "forms": forms, "src": len(src), "dst": len(dst), "bbox_diagonal": diag, "max_dist": max_dist,
              "cell": cell, "planted": {"angle_degrees": args.angle, "shift": args.shift * max_dist, "T": planted.tolist()},
              "normals": {"k": args.normals_k, "n_valid": info["n_valid"], "max_dist": info["max_dist"], "ms": med["normals_ms"]},
              "all_rounds": rows, **med, "plane_over_pair_moments": med["plane_moments_ms"] / med["pair_moments_ms"]}
    for name in ("point", "plane"):
        r = ref[name]
        result[name] = {"iterations": r["iterations"], "converged": r["converged"], "fitness": r["fitness"], "rmse": r["rmse"],
                        "rmse_point": r.get("rmse_point", r["rmse"]), "history": r["history"], "T": r["T"].tolist(),
                        "total_ms": med[name + "_total_ms"], "ms_per_iteration": med[name + "_total_ms"] / r["iterations"],
                        "recovery_error": recovery(r["T"]), "recovery_error_over_max_dist": recovery(r["T"]) / max_dist}
    result["point_over_plane_iterations"] = ref["point"]["iterations"] / ref["plane"]["iterations"]
    result["point_over_plane_total_ms"] = med["point_total_ms"] / med["plane_total_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    for name in ("point", "plane"):
        print(json.dumps({"method": name, **{k: v for k, v in result[name].items() if k not in ("history", "T")}}))
    print(json.dumps({k: result[k] for k in ("normals", "pair_moments_ms", "plane_moments_ms", "plane_over_pair_moments", "point_over_plane_iterations",
                                             "point_over_plane_total_ms")} | {"out": args.out}))


if __name__ == "__main__":
    main()
