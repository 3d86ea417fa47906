"""A scan to its point cloud, two paths, same process, interleaved: (a) the file pipeline - `inference_scan` -> PFMs -> `fusion.fusion()` (read the PFMs
back, upload the depth stack, vote loop, masks and averaged depths to the host, float64 numpy back-projection) - and (b) `scan.reconstruct_scan`
(everything between the images and the point cloud stays on the device).

    python tools/bench_reconstruct.py [--views 49] [--size 1184x1600] [--neighbours 10] [--rounds 3] [--out profiles/reconstruct_bench.json]
    python tools/bench_reconstruct.py --kernels        # the point-cloud passes alone (11 views of 1184x1600, mask area 0.25): HIP-event times;
                                                       # run this form under `rocprofv3 --kernel-trace --stats -- python ...` for per-kernel figures
    python tools/bench_reconstruct.py --kernel-stats FILE.csv --out profiles/reconstruct_bench.json     # merge that run's kernel rows into the JSON

The synthetic scan of tools/bench_scan.py (seeded, ring neighbours).  One warm-up of each path, then `--rounds` rounds of (a) then (b); medians.  Wall
times end in a device synchronise and are split into depth maps / vote loop / tail (for (a) the tail is everything of fusion() outside the loop: PFM
read-back, upload, device->host copies, back-projection, PLY and mask files).  Bytes over PCIe are counted from the tensor sizes.  Needs a GPU."""
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

from bench_scan import ring_pairs  # noqa: E402


def bench_kernels(dev, reps=20, warmup=5):
    """count + scan and emit at 11 views of 1184x1600, mask area 0.25, HIP events around the two C calls (buffers and cameras prepared before;
    the host read of the per-view totals between them is not inside either span), against their compulsory bytes: count reads 1 B per pixel;
    emit reads 5 B per pixel (mask + depth) and 12 B of colour planes per point and writes 15 B per point"""
    import ctypes
    from cer_mvs_amd import _lib as L, fusion
    from cer_mvs_amd.synthetic import synthetic_scene
    N, h, w = 11, 1184, 1600
    _, poses, intr, _ = synthetic_scene(32, 32, N - 1, seed=3)
    g = torch.Generator(device=dev).manual_seed(5)
    masks = (torch.rand(N, h, w, device=dev, generator=g) < 0.25).to(torch.uint8)
    est = 0.4 + 2.0 * torch.rand(N, h, w, device=dev, generator=g)
    col = torch.rand(N, 3, h, w, device=dev, generator=g)
    cams = fusion.cloud_cams(intr[0].float(), poses[0].float()).to(dev)
    lib = L.load()
    order = (ctypes.c_int * N)(*range(N))
    P = int(lib.cer_cloud_partials(N, h, w))
    partials = torch.empty(P, device=dev, dtype=torch.int32)
    offsets = torch.empty(P + 1, device=dev, dtype=torch.int64)
    view_base = torch.empty(N + 1, device=dev, dtype=torch.int64)
    n = int(masks.sum())
    xyz = torch.empty(n, 3, device=dev, dtype=torch.float32)
    rgb = torch.empty(n, 3, device=dev, dtype=torch.uint8)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    t_count, t_emit = [], []
    for k in range(warmup + reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        L.check(lib.cer_cloud_count_u8(p(masks), N, h, w, order, N, p(partials), p(offsets), p(view_base), L.cur_stream()), "cloud_count")
        ev[1].record()
        assert int(view_base.cpu()[-1]) == n
        ev[2].record()
        L.check(lib.cer_cloud_emit_f32(p(masks), p(est), p(cams), p(col), N, h, w, order, N, p(offsets), n, n, p(xyz), p(rgb), L.cur_stream()),
                "cloud_emit")
        ev[3].record()
        torch.cuda.synchronize()
        if k >= warmup:
            t_count.append(ev[0].elapsed_time(ev[1]))
            t_emit.append(ev[2].elapsed_time(ev[3]))
    b_count, b_emit = N * h * w, 5 * N * h * w + 27 * n
    mc, me = statistics.median(t_count), statistics.median(t_emit)
    return {"views": N, "height": h, "width": w, "points": n, "reps": reps, "warmup": warmup,
            "count_scan_ms_median": mc, "count_scan_ms_min": min(t_count), "emit_ms_median": me, "emit_ms_min": min(t_emit),
            "count_compulsory_bytes": b_count, "emit_compulsory_bytes": b_emit,
            "count_scan_fraction_of_8TBps": b_count / (mc * 1e-3) / 8e12, "emit_fraction_of_8TBps": b_emit / (me * 1e-3) / 8e12,
            "all_fraction_of_8TBps": (b_count + b_emit) / ((mc + me) * 1e-3) / 8e12}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--size", default="1184x1600", help="HxW of the images")
    ap.add_argument("--neighbours", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3, help="timed rounds of (a) then (b), after one warm-up of each")
    ap.add_argument("--iters", type=int, default=16, help="GRU iterations per cascade stage")
    ap.add_argument("--kernels", action="store_true", help="only the point-cloud passes at full size")
    ap.add_argument("--kernel-stats", help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of the --kernels form: its cloud / colour / depth "
                    "kernel rows are merged into --out")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "reconstruct_bench.json"))
    args = ap.parse_args()
    if args.kernel_stats:
        import csv
        rows = [r for r in csv.DictReader(open(args.kernel_stats)) if any(k in r.get("Name", "") for k in ("cloud_", "color_grid", "disp_to_depth"))]
        result = json.load(open(args.out))
        result["rocprofv3_kernel_stats"] = [{k: r[k] for k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs") if k in r} for r in rows]
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps(result["rocprofv3_kernel_stats"]))
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_reconstruct: needs a GPU")
    dev = torch.device("cuda:0")
    if args.kernels:
        print(json.dumps(bench_kernels(dev)))
        return
    from cer_mvs_amd import RAFT
    from cer_mvs_amd import fusion as FU
    from cer_mvs_amd.scan import inference_scan, reconstruct_scan
    from cer_mvs_amd.synthetic import fill_state_dict, synthetic_scene

    H, W = (int(v) for v in args.size.lower().split("x"))
    M, nb = args.views, args.neighbours
    model = RAFT(cascade=[(64, 64, args.iters), (-1, 320, args.iters)], test_mode=True)
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=5))
    model = model.to(dev).eval()
    t0 = time.perf_counter()
    images, poses, intr, scale = synthetic_scene(H, W, M - 1, seed=0)
    images, poses, intr = images[0].contiguous(), poses[0], intr[0]
    print(f"scene: {M} views of {W}x{H} in {time.perf_counter() - t0:.1f} s", flush=True)
    names = [f"{i:08d}" for i in range(M)]
    pairs = ring_pairs(M, nb)
    scales = [scale] * M
    h, w = H // 4, W // 4
    # fusion() takes the reference view's image and cameras from each item, and the names of its source views
    loader = [(images[i:i + 1][None], poses[i:i + 1][None], intr[i:i + 1][None], [(names[j],) for j in [i] + pairs[i]], None) for i in range(M)]
    plain_fuse = FU.fuse_depth_maps
    marks = {}

    def timed_fuse(*a, **k):
        marks["loop0"] = time.perf_counter()
        out = plain_fuse(*a, **k)
        torch.cuda.synchronize()
        marks["loop1"] = time.perf_counter()
        return out

    def run_files(folder):
        t = time.perf_counter()
        inference_scan(model, images, poses, intr, names, pairs, scales, folder, num_frames=nb, streams=3)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        FU.fuse_depth_maps = timed_fuse
        try:
            out = FU.fusion(loader, folder, suffix=f"_scale1_nf{nb}", glb=0.25)
        finally:
            FU.fuse_depth_maps = plain_fuse
        t2 = time.perf_counter()
        n = len(out["xyz"])
        return {"wall_s": t2 - t, "depths_s": t1 - t, "fuse_s": marks["loop1"] - marks["loop0"], "tail_s": (t2 - t1) - (marks["loop1"] - marks["loop0"]),
                "points": n, "h2d_bytes": M * 3 * H * W * 4 + M * h * w * 4, "d2h_bytes": M * h * w * 4 + M * h * w * 5}

    def run_device(folder):
        tm = {}
        t = time.perf_counter()
        out = reconstruct_scan(model, images, poses, intr, names, pairs, scales, folder, num_frames=nb, glb=0.25, streams=3, timings=tm)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t
        return {"wall_s": wall, "depths_s": tm["depths_s"], "fuse_s": tm["fuse_s"], "tail_s": tm["tail_s"], "points": len(out["xyz"]),
                "h2d_bytes": M * 3 * H * W * 4, "d2h_bytes": tm["d2h_bytes"]}

    result = {"views": M, "height": H, "width": W, "neighbours": nb, "gru_iterations": 2 * args.iters, "rounds": args.rounds,
              "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as tmp:
        fa, fb = os.path.join(tmp, "a"), os.path.join(tmp, "b")
        run_files(fa)                                        # warm-up (also: calibration of gru_precision="auto")
        run_device(fb)
        ra, rb = [], []
        for _ in range(args.rounds):
            ra.append(run_files(fa))
            rb.append(run_device(fb))
    for name, runs in (("file_pipeline", ra), ("reconstruct_scan", rb)):
        med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
        med["all_wall_s"] = [round(r["wall_s"], 4) for r in runs]
        result[name] = med
        print(f"{name}: wall {med['wall_s']:.3f} s (depth maps {med['depths_s']:.3f}, vote loop {med['fuse_s']:.3f}, tail {med['tail_s']:.3f}), "
              f"{med['points']} points, PCIe {med['h2d_bytes'] / 1e6:.1f} MB up / {med['d2h_bytes'] / 1e6:.1f} MB down", flush=True)
    result["reconstruct_over_files"] = result["reconstruct_scan"]["wall_s"] / result["file_pipeline"]["wall_s"]
    result["point_cloud_full_size"] = bench_kernels(dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"reconstruct_over_files": result["reconstruct_over_files"], "point_cloud_full_size": result["point_cloud_full_size"], "out": args.out}))


if __name__ == "__main__":
    main()
