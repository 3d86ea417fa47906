"""A whole scan, three drivers, same process: `inference()` as it is (a list-backed loader hands it one stack per reference view),
`inference_scan` with the feature store switched off (device-side preparation and the single upload only) and `inference_scan` cached.

    python tools/bench_scan.py [--views 49] [--size 1184x1600] [--neighbours 10] [--scans 3] [--out profiles/scan_bench.json]

A synthetic scan (synthetic_scene, seeded) of `--views` images; every image is the reference view once, with its `--neighbours` ring
neighbours as source views.  Per driver and per `streams` in (1, 3): one warm-up scan, then the median wall time of `--scans` scans
(each ends with the last depth map written: every timing ends in a device synchronise), and the host parts timed on their own - the
loader's stack gather (NOT counted against `inference()`: a real loader prefetches it in worker processes), the CPU resize inside
`inference()`, the session's upload + preparation and its encode.  Last, the GPU-side time per depth map on resident data: `RAFT.forward` on a
resident stack against `ScanSession.depth`, one at a time and three in flight.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402


def ring_pairs(M, n):
    """source views of reference view i: its n nearest ring neighbours, nearest first (+1, -1, +2, -2, ...)"""
    out = []
    for i in range(M):
        nb, d = [], 1
        while len(nb) < n:
            for j in ((i + d) % M, (i - d) % M):
                if j != i and j not in nb and len(nb) < n:
                    nb.append(j)
            d += 1
        out.append(nb)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--size", default="1184x1600", help="HxW of the images")
    ap.add_argument("--neighbours", type=int, default=10)
    ap.add_argument("--scans", type=int, default=3, help="timed scans per driver and stream count (>= 3), after one warm-up scan")
    ap.add_argument("--iters", type=int, default=16, help="GRU iterations per cascade stage (bench.py's DTU workload: 16 + 16)")
    ap.add_argument("--resident-steps", type=int, default=30, help="depth maps of the resident-data timing")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scan_bench.json"))
    args = ap.parse_args()
    if args.scans < 3:
        ap.error("--scans must be at least 3")
    if not torch.cuda.is_available():
        raise SystemExit("bench_scan: needs a GPU")
    from cer_mvs_amd import RAFT
    from cer_mvs_amd import inference as inf_mod
    from cer_mvs_amd.scan import ScanSession, inference_scan
    from cer_mvs_amd.synthetic import fill_state_dict, synthetic_scene

    H, W = (int(v) for v in args.size.lower().split("x"))
    M, nb = args.views, args.neighbours
    dev = torch.device("cuda:0")
    cascade = [(64, 64, args.iters), (-1, 320, args.iters)]
    model = RAFT(cascade=cascade, test_mode=True)
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=5))
    model = model.to(dev).eval()
    t0 = time.perf_counter()
    images, poses, intr, scale = synthetic_scene(H, W, M - 1, seed=0)
    images, poses, intr = images[0].contiguous(), poses[0], intr[0]
    print(f"scene: {M} views of {W}x{H} in {time.perf_counter() - t0:.1f} s", flush=True)
    names = [f"{i:08d}" for i in range(M)]
    pairs = ring_pairs(M, nb)
    scales = [scale] * M
    host = {"loader_s": 0.0, "resize_s": 0.0}

    def loader():
        for i in range(M):
            t = time.perf_counter()
            idx = [i] + pairs[i]
            item = (images[idx][None], poses[idx][None], intr[idx][None], [names[i]], scales[i])
            host["loader_s"] += time.perf_counter() - t
            yield item

    plain_scale = inf_mod.scale_operation

    def timed_scale(*a, **k):
        t = time.perf_counter()
        out = plain_scale(*a, **k)
        host["resize_s"] += time.perf_counter() - t
        return out

    def run_inference(streams, folder):
        host["loader_s"] = host["resize_s"] = 0.0
        inf_mod.scale_operation = timed_scale
        try:
            t = time.perf_counter()
            inf_mod.inference(loader(), None, folder, model=model, num_frames=nb, streams=streams)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t
        finally:
            inf_mod.scale_operation = plain_scale
        return {"wall_s": wall, "loader_s": host["loader_s"], "resize_s": host["resize_s"], "scan_s": wall - host["loader_s"]}

    def run_scan(streams, folder, force_uncached):
        tm = {}
        t = time.perf_counter()
        inference_scan(model, images, poses, intr, names, pairs, scales, folder, num_frames=nb, streams=streams,
                       force_uncached=force_uncached, timings=tm)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t
        assert tm["cached"] == (not force_uncached), tm
        return {"wall_s": wall, "scan_s": wall, "upload_prep_s": tm.get("upload_prep_s", 0.0), "encode_s": tm.get("encode_s", 0.0)}

    drivers = {"inference": lambda s, f: run_inference(s, f), "scan_uncached": lambda s, f: run_scan(s, f, True),
               "scan_cached": lambda s, f: run_scan(s, f, False)}
    result = {"views": M, "height": H, "width": W, "neighbours": nb, "gru_iterations": 2 * args.iters, "scans": args.scans,
              "device": torch.cuda.get_device_name(0), "drivers": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for streams in (1, 3):
            for name, run in drivers.items():
                run(streams, os.path.join(tmp, name))                          # warm-up scan (also: calibration of gru_precision="auto")
                runs = [run(streams, os.path.join(tmp, name)) for _ in range(args.scans)]
                med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
                med["ms_per_depth_map"] = 1e3 * med["scan_s"] / M
                med["all_scan_s"] = [round(r["scan_s"], 4) for r in runs]
                result["drivers"][f"{name}_streams{streams}"] = med
                print(f"{name} streams={streams}: {med['ms_per_depth_map']:.2f} ms per depth map "
                      f"({', '.join(f'{k} {v:.3f}' for k, v in med.items() if k.endswith('_s') and k != 'all_scan_s')})", flush=True)

    # ---- GPU-side time per depth map on resident data
    resident = {}
    n = args.resident_steps
    for streams in (1, 3):
        sess = ScanSession(model, images, poses, intr, streams=streams)
        stacks = [(sess.stack(i, pairs[i]), sess.poses[[i] + pairs[i]][None], sess.intrinsics[[i] + pairs[i]][None]) for i in range(3)]

        def fwd_loop():
            hs = [sess.pipe.submit(*stacks[k % 3], scale) for k in range(n)]
            for h_ in hs:
                sess.pipe.result(h_)

        def depth_loop():
            hs = [sess.submit(k % M, pairs[k % M], scale) for k in range(n)]
            for h_ in hs:
                sess.result(h_)

        for label, loop in (("forward_resident", fwd_loop), ("depth_cached", depth_loop)):
            loop()
            torch.cuda.synchronize()
            times = []
            for _ in range(3):
                t = time.perf_counter()
                loop()
                torch.cuda.synchronize()
                times.append(1e3 * (time.perf_counter() - t) / n)
            resident[f"{label}_streams{streams}_ms"] = statistics.median(times)
        resident[f"encode_ms_per_image_streams{streams}"] = 1e3 * sess.timings.get("encode_s", 0.0) / M
        assert sess.cached
        sess.close()
    result["resident"] = resident
    for k, v in resident.items():
        print(f"{k}: {v:.3f}", flush=True)
    d = result["drivers"]
    result["cached_over_inference"] = {f"streams{s}": d[f"inference_streams{s}"]["ms_per_depth_map"] / d[f"scan_cached_streams{s}"]["ms_per_depth_map"]
                                       for s in (1, 3)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"cached_over_inference": result["cached_over_inference"], "out": args.out}))


if __name__ == "__main__":
    main()
