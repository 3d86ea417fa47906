#!/usr/bin/env python3
"""Time one whole training step (cer_mvs_amd.train.train_step) with backend="torch" and backend="hip", alternating, on the
reference's DTU training shape: crop 1056x1440 (configs/train_DTU.gin), 10 source views (datasets/dtu.py num_frames=10), cascade
(64,64,8),(-1,320,8) - RAFT's default.  Batch 1 (the package's), fp32 forward, GradScaler on, AdamW + OneCycleLR.

Per backend: milliseconds per step (host clock around a step that ends in a device synchronise, median and spread over the timed
steps) and the peak allocated memory of a step.  Kernel times come from a separate profiled run:

  rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/bench_train.py --steps 2 --warmup 1
  python tools/bench_train.py --kernel-stats OUT/.../run_results.db --steps 2 --warmup 1

prints the rows of the lookup and upsample kernels of both backends (HIP: train_lookup_*, upsample_ac_*; torch: grid_sampler_2d*,
avg_pool2d*, upsample_bilinear2d*).  Needs a GPU: there is no CPU timing."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

KERNELS = {"hip": ("train_lookup_fwd", "train_lookup_bwd", "upsample_ac_fwd", "upsample_ac_bwd"),
           "torch": ("grid_sampler_2d", "avg_pool2d", "upsample_bilinear2d")}


def kernel_stats(path, steps):
    """Rows of the lookup / upsample kernels: calls, total and per-step milliseconds (``steps``: train_steps per backend in the profiled
    run, warm-up included), mean microseconds per call.  ``path``: rocprofv3's rocpd database (``*_results.db``) or its kernel_stats.csv."""
    acc = {}
    if path.endswith(".db"):
        import sqlite3
        con = sqlite3.connect(path)
        for name, t0, t1 in con.execute("select name, start, end from kernels"):
            a = acc.setdefault(name, [0, 0.0])
            a[0] += 1
            a[1] += (t1 - t0)
    else:
        with open(path) as f:
            for r in csv.DictReader(f):
                acc[r.get("Name") or r.get("KernelName") or ""] = [int(r["Calls"]), float(r["TotalDurationNs"])]
    rows = {}
    for name, (calls, ns) in sorted(acc.items(), key=lambda kv: -kv[1][1]):
        for backend, keys in KERNELS.items():
            if any(k in name for k in keys):
                rows[name[:100]] = {"backend": backend, "calls": calls, "ms_per_step": round(ns / 1e6 / steps, 3),
                                    "us_per_call": round(ns / 1e3 / calls, 1)}
    for backend in KERNELS:
        rows["total " + backend] = {"ms_per_step": round(sum(r["ms_per_step"] for r in rows.values() if r.get("backend") == backend), 3)}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5, help="timed steps per backend")
    ap.add_argument("--warmup", type=int, default=2, help="untimed steps per backend first")
    ap.add_argument("--H", type=int, default=1056)
    ap.add_argument("--W", type=int, default=1440)
    ap.add_argument("--views", type=int, default=10, help="source views")
    ap.add_argument("--backends", default="torch,hip")
    ap.add_argument("--out", default=None, help="also write the JSON record here")
    ap.add_argument("--kernel-stats", default=None, help="summarise a rocprofv3 results .db / kernel_stats.csv and exit "
                    "(with the --steps / --warmup of the profiled run)")
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps(kernel_stats(a.kernel_stats, a.steps + a.warmup), indent=1))
        return
    import torch
    from cer_mvs_amd import RAFT
    from cer_mvs_amd.synthetic import fill_state_dict, synthetic_scene
    from cer_mvs_amd.train import fetch_optimizer, train_step
    if not torch.cuda.is_available():
        raise SystemExit("bench_train: needs a GPU")
    dev = torch.device("cuda:0")
    cascade = [(64, 64, 8), (-1, 320, 8)]
    images, poses, intr, _ = synthetic_scene(a.H, a.W, a.views, seed=0)
    model = RAFT(cascade=cascade, test_mode=False)
    model.load_state_dict(fill_state_dict(model.state_dict(), seed=5))
    model = model.to(dev).train()
    optimizer, scheduler = fetch_optimizer(model, num_steps=100000)
    scaler = torch.amp.GradScaler("cuda", enabled=True)
    # ground truth: the plane the synthetic scene renders, with an invalid band (depth 0) like DTU's masked pixels
    depths = torch.full((1, a.views + 1, a.H, a.W), 600.0, device=dev)
    depths[:, :, : a.H // 8] = 0.0
    images, poses, intr = images.to(dev), poses.to(dev), intr.to(dev)
    backends = a.backends.split(",")
    times = {b: [] for b in backends}
    peak = {b: 0 for b in backends}
    losses = {b: [] for b in backends}

    def step(b):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        loss, _m = train_step(model, optimizer, scheduler, scaler, images, depths, poses, intr, 0.3, backend=b)
        loss = float(loss.detach())
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        peak[b] = max(peak[b], torch.cuda.max_memory_allocated())
        losses[b].append(loss)
        return dt

    for _ in range(a.warmup):
        for b in backends:
            step(b)
    for _ in range(a.steps):
        for b in backends:                                   # alternating: both backends see the same box state
            times[b].append(step(b))
    rec = {"shape": {"H": a.H, "W": a.W, "source_views": a.views, "cascade": cascade, "batch": 1},
           "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    for b in backends:
        ms = [1e3 * t for t in times[b]]
        rec[b] = {"ms_per_step_median": round(statistics.median(ms), 2) if ms else None,
                  "ms_per_step_min": round(min(ms), 2) if ms else None, "ms_per_step_max": round(max(ms), 2) if ms else None,
                  "peak_alloc_MiB": round(peak[b] / 2 ** 20, 1), "losses": losses[b]}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
