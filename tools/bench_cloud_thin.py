"""Greedy radius thinning (cloud_eval.radius_thin) on the cloud the project itself produces: the synthetic scan of
tools/bench_cloud_eval.py goes through `reconstruct_scan` in the default arithmetic form (the cloud that is thinned) and with
gru_precision="s16" (the cloud that is evaluated against it).

    python tools/bench_cloud_thin.py [--views 49] [--size 1184x1600] [--radii 0.125,0.25,0.5] [--rounds 3] [--host-subset 0]
                                     [--out profiles/cloud_thin_bench.json]

Radii are fractions of max_dist = 1 % of the default cloud's bounding-box diagonal (bench_cloud_eval's cut-off).  Per radius, order="random",
seed 0, cell = radius: (1) radius_thin as a whole between HIP events (index build in visiting order, rounds, compactions, the final gather),
median of --rounds runs, and the same with THIN_ROUNDS_PER_COMPACTION = 1, 2, 4; (2) one instrumented run of the same loop, written out
here, with events around the index build, every round and every compaction; (3) the kept count beside voxel_downsample's at cell = radius, and
the closest pair among each selection and the points left without a kept point within the radius; (4) the comparator: the sequential greedy on the host over scipy.spatial.cKDTree.query_ball_point (host clock, tree build
apart), on the first --host-subset points of the visiting order (0: the whole cloud) - the figure is labelled with that count, nothing is
extrapolated - and the device on the same sub-cloud in the same order, whose kept set is compared with the host's; (5) accuracy_completeness
of the s16 cloud against the default cloud, the s16 cloud thinned under both methods.  Needs a GPU."""
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


def instrumented(CE, points, radius, seed):
    """radius_thin's loop (order="random", cell = radius) with events around its parts -> dict of times; the kept set is checked against
    radius_thin's by the caller"""
    from cer_mvs_amd import _lib as L
    lib, dev = L.load(), points.device
    ev = lambda: torch.cuda.Event(enable_timing=True)
    marks = [("start", ev())]
    marks[0][1].record()

    def mark(name):
        e = ev()
        e.record()
        marks.append((name, e))
    visit = torch.randperm(len(points), generator=torch.Generator("cpu").manual_seed(seed)).to(dev)
    pts = points.index_select(0, visit)
    mark("permute")
    index = CE.CloudIndex(pts, radius)
    mark("build")
    state = torch.zeros(len(points), device=dev, dtype=torch.uint8)
    P = int(lib.cer_grid_partials(index.n))
    partials, offsets = torch.empty(P, device=dev, dtype=torch.int32), torch.empty(P + 1, device=dev, dtype=torch.int64)
    total = torch.empty(1, device=dev, dtype=torch.int64)
    lists = [torch.empty(index.n, device=dev, dtype=torch.int32) for _ in range(2)]
    rec, ck, cs = (L.dev_ptr(index.records, "records", torch.int32), L.dev_ptr(index.cell_keys, "cell_keys", torch.int64),
                   L.dev_ptr(index.cell_start, "cell_start", torch.int64))
    ps = L.dev_ptr(state, "state", torch.uint8)
    active, n_active, comp, sizes = None, index.n, 0, []
    mark("alloc")
    while n_active:
        pa = L.dev_ptr(active, "active", torch.int32)
        for _ in range(CE.THIN_ROUNDS_PER_COMPACTION):
            L.check(lib.cer_grid_thin_round_f32(rec, index.n, ck, cs, index.cells, index.origin, index.cell, pa, n_active, radius, ps,
                                                L.cur_stream()), "grid_thin_round")
            mark("round")
            sizes.append(n_active)
        out = lists[comp & 1]
        L.check(lib.cer_grid_thin_compact_i32(rec, index.n, ps, pa, n_active, L.dev_ptr(partials, "partials", torch.int32),
                                              L.dev_ptr(offsets, "offsets", torch.int64), L.dev_ptr(out, "out", torch.int32),
                                              L.dev_ptr(total, "total", torch.int64), L.cur_stream()), "grid_thin_compact")
        comp += 1
        active, n_active = out, int(total.cpu())
        mark("compact")                                      # (the compaction's three launches and the host's read of the total)
    kept = torch.sort(visit.index_select(0, torch.nonzero(state == 1).flatten())).values
    mark("gather")
    torch.cuda.synchronize()
    ms = {}
    for (_, e0), (name, e1) in zip(marks, marks[1:]):
        ms.setdefault(name, []).append(e0.elapsed_time(e1))
    return kept, {"permute_ms": ms["permute"][0], "build_ms": ms["build"][0], "round_ms": ms["round"], "active_list": sizes,
                  "compact_ms": ms["compact"], "gather_ms": ms["gather"][0], "rounds_total_ms": sum(ms["round"]),
                  "compactions_total_ms": sum(ms["compact"]), "total_ms": marks[0][1].elapsed_time(marks[-1][1]), "cells": index.cells}


def closest_pair(pts):
    """smallest distance between two different points of ``pts`` (None below two points): scipy's k = 2 query on the host, fp64 - nearest()
    of a cloud in itself finds the point itself"""
    from scipy.spatial import cKDTree
    P = pts.double().cpu().numpy()
    if len(P) < 2:
        return None
    return float(cKDTree(P).query(P, k=2, workers=16)[0][:, 1].min())


def host_greedy(P64, radius, visit):
    """the sequential loop on the host -> (kept indices ascending, tree build s, loop s)"""
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    tree = cKDTree(P64)
    t1 = time.perf_counter()
    alive, kept = np.isfinite(P64).all(1), []
    for i in visit:
        if alive[i]:
            kept.append(i)
            alive[tree.query_ball_point(P64[i], radius)] = False
    t2 = time.perf_counter()
    return np.sort(np.asarray(kept, np.int64)), t1 - t0, t2 - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--size", default="1184x1600", help="HxW of the images")
    ap.add_argument("--neighbours", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=16, help="GRU iterations per cascade stage")
    ap.add_argument("--radii", default="0.125,0.25,0.5", help="fractions of max_dist")
    ap.add_argument("--host-subset", type=int, default=0, help="points of the visiting order the host comparator runs on (0: all)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cloud_thin_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cloud_thin: needs a GPU")
    dev = torch.device("cuda:0")
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
    cloud, other = clouds["default"], clouds["s16"]
    diag = float((cloud.amax(0) - cloud.amin(0)).double().norm())
    max_dist = float(np.float32(0.01 * diag))
    result = {"views": M, "height": H, "width": W, "neighbours": nb, "gru_iterations": 2 * args.iters, "rounds": args.rounds,
              "device": torch.cuda.get_device_name(0), "forms": forms, "points": len(cloud), "points_s16": len(other), "bbox_diagonal": diag,
              "max_dist": max_dist, "order": "random", "seed": 0, "rounds_per_compaction": CE.THIN_ROUNDS_PER_COMPACTION, "radii": []}
    default_k = CE.THIN_ROUNDS_PER_COMPACTION
    visit = torch.randperm(len(cloud), generator=torch.Generator("cpu").manual_seed(0))
    for frac in (float(v) for v in args.radii.split(",")):
        radius = float(np.float32(frac * max_dist))
        row = {"radius": radius, "radius_over_max_dist": frac}
        info = {}
        kept = CE.radius_thin(cloud, radius, info=info)      # warm-up, and the set every other path is compared with
        row.update(info, kept=len(kept))
        sweep = {}
        for k in (1, 2, 4):
            CE.THIN_ROUNDS_PER_COMPACTION = k
            ms, inf = [], {}
            for _ in range(args.rounds):
                got, t = timed(lambda: CE.radius_thin(cloud, radius, info=inf))
                ms.append(t)
                assert torch.equal(got, kept)
            sweep[str(k)] = {"total_ms": statistics.median(ms), "all_rounds_ms": ms, "rounds": inf["rounds"], "compactions": inf["compactions"]}
        CE.THIN_ROUNDS_PER_COMPACTION = default_k
        row["rounds_per_compaction_sweep"] = sweep
        row["total_ms"] = sweep[str(default_k)]["total_ms"]
        got, parts = instrumented(CE, cloud, radius, 0)
        assert torch.equal(got, kept)
        row["instrumented"] = parts
        # the two thinnings side by side
        vox, vox_ms = timed(lambda: CE.voxel_downsample(cloud, radius))
        row["voxel"] = {"kept": len(vox), "ms": vox_ms, "closest_pair": closest_pair(cloud.index_select(0, vox))}
        row["closest_pair"] = closest_pair(cloud.index_select(0, kept))
        d = CE.CloudIndex(cloud.index_select(0, kept), radius).nearest(cloud, radius)[0]
        row["points_without_a_kept_point_within_radius"] = int(torch.isinf(d).sum())
        d = CE.CloudIndex(cloud.index_select(0, vox), radius).nearest(cloud, radius)[0]
        row["voxel"]["points_without_a_kept_point_within_radius"] = int(torch.isinf(d).sum())
        # the comparator: sequential greedy on the host, on the first `sub` points of the visiting order
        sub = len(cloud) if args.host_subset <= 0 else min(args.host_subset, len(cloud))
        members = visit[:sub]
        sub_cloud = cloud.index_select(0, members.to(dev))   # its own order IS the visiting order
        want, build_s, loop_s = host_greedy(sub_cloud.double().cpu().numpy(), radius, np.arange(sub))
        inf = {}
        got, dev_ms = timed(lambda: CE.radius_thin(sub_cloud, radius, order="index", info=inf))
        _, dev_ms = timed(lambda: CE.radius_thin(sub_cloud, radius, order="index", info=inf))
        row["host_comparator"] = {"what": "sequential greedy over scipy.spatial.cKDTree.query_ball_point, one thread, host clock",
                                  "points": sub, "is_the_whole_cloud": sub == len(cloud), "kept": len(want), "tree_build_ms": 1e3 * build_s,
                                  "loop_ms": 1e3 * loop_s, "total_ms": 1e3 * (build_s + loop_s),
                                  "device_same_points_ms": dev_ms, "device_rounds": inf["rounds"],
                                  "host_over_device": 1e3 * (build_s + loop_s) / dev_ms,
                                  "kept_sets_equal": bool(np.array_equal(got.cpu().numpy(), want))}
        # the protocol: the s16 cloud, thinned, against the default cloud
        row["dtu_s16_vs_default"] = {m: CE.accuracy_completeness(other, cloud, max_dist=max_dist, thin=radius, thin_method=m)
                                     for m in ("voxel", "greedy")}
        result["radii"].append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "instrumented"}), flush=True)
    result["dtu_s16_vs_default_unthinned"] = CE.accuracy_completeness(other, cloud, max_dist=max_dist)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
