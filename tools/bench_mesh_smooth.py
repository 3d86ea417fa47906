"""Mesh edges, the topology report and Taubin smoothing on the 513^3 sphere case of tools/bench_mesh.py: ten analytic views
of a unit sphere at 1600x1184, the mesh of `mesh_from_depth_maps` on a cubic grid of --resolution + 1 nodes per axis (2.58 M vertices and
5.15 M faces at 512).

    python tools/bench_mesh_smooth.py [--size 1184x1600] [--resolution 512] [--rounds 3] [--out profiles/mesh_smooth_bench.json]

Between HIP events, medians of --rounds interleaved rounds after a warm-up: the stages of `mesh_edges` (the keys kernel, the sort, count /
scan / emit with its host read, the binary search for `nbr_starts`), `mesh_topology`, `smooth_mesh`'s prepare, ONE smoothing step (with the
bytes it must move at least - every array read or written once - against the HBM peak of 8 TB/s), the finish, and a Taubin x 10 call on the
host clock.  Beside them the same contract restated in torch ops on the device (`torch.unique` on the edge keys, `index_add_` for the
sums): its edge table compared exactly, its step by the largest difference (its sums are atomic, so its bits differ from run to run).
Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from bench_cloud_eval import timed  # noqa: E402
from bench_mesh import SPHERE_DIRS, sphere_scene  # noqa: E402

HBM_PEAK = 8.0e12                                            # bytes per second, the MI355X's specified peak


def torch_edges(fac, nv):
    """the undirected edge table in torch ops: (lo, hi, n_lo_hi, n_hi_lo)"""
    f = fac.long()
    a = torch.cat([f[:, 0], f[:, 1], f[:, 2]])
    b = torch.cat([f[:, 1], f[:, 2], f[:, 0]])
    keep = a != b
    a, b = a[keep], b[keep]
    lo, hi = torch.minimum(a, b), torch.maximum(a, b)
    uniq, inv = torch.unique(lo * nv + hi, return_inverse=True)
    fw = torch.bincount(inv[a < b], minlength=uniq.shape[0])
    bw = torch.bincount(inv[a > b], minlength=uniq.shape[0])
    return (uniq // nv).int(), (uniq % nv).int(), fw.int(), bw.int()


def torch_step(p, lo, hi, w):
    """one step on fp64 positions over the edge table (finite vertices, free boundary): index_add_ sums, atomic"""
    s = torch.zeros_like(p).index_add_(0, lo, p[hi]).index_add_(0, hi, p[lo])
    n = torch.zeros(p.shape[0], device=p.device, dtype=torch.float64).index_add_(0, lo, torch.ones_like(lo, dtype=torch.float64))
    n.index_add_(0, hi, torch.ones_like(hi, dtype=torch.float64))
    return torch.where((n > 0)[:, None], p + w * (s / n.clamp(min=1.0)[:, None] - p), p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1184x1600", help="HxW of the sphere's depth maps")
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_smooth_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_smooth: needs a GPU")
    dev = torch.device("cuda:0")
    from cer_mvs_amd import _lib as L
    from cer_mvs_amd import mesh as ME

    H, W = (int(v) for v in args.size.lower().split("x"))
    res = args.resolution
    depths, masks, Ks, Es = sphere_scene(H, W, dev)
    voxel = 2.4 / res
    grid = ME.Grid((-1.2 + 0.013 * voxel,) * 3, voxel, (res + 1,) * 3)
    ver, fac = ME.mesh_from_depth_maps(depths, masks, Ks, Es, grid, trunc=3.0 * voxel)
    del depths, masks
    torch.cuda.empty_cache()
    lib, st = L.load(), L.cur_stream()
    nv, nf = int(ver.shape[0]), int(fac.shape[0])
    p = lambda t, dt=torch.float32: L.dev_ptr(t, "t", dt)

    starts, nbrs, along, against = ME.mesh_edges(fac, nv)
    nn = int(nbrs.shape[0])
    report = ME.mesh_topology(fac, nv)
    print(f"{nv} vertices, {nf} faces, {nn // 2} edges; {report}", flush=True)
    info = {}
    smoothed = ME.smooth_mesh(ver, fac, 10, info=info)
    dist = lambda x: {"mean": float((x.double().norm(dim=1) - 1.0).abs().mean()), "max": float((x.double().norm(dim=1) - 1.0).abs().max())}

    P = int(lib.cer_mesh_edge_partials(nf))
    keys = torch.empty(6 * nf, device=dev, dtype=torch.int64)
    partials = torch.empty(P, device=dev, dtype=torch.int32)
    offsets = torch.empty(P + 2, device=dev, dtype=torch.int64)
    totals = torch.zeros(2, device=dev, dtype=torch.int64)
    owner, e_nbrs, e_along, e_against = (torch.empty(nn, device=dev, dtype=torch.int32) for _ in range(4))
    walk = torch.empty(nn, device=dev, dtype=torch.int32)
    flags = torch.zeros(nv, device=dev, dtype=torch.uint8)
    state = torch.empty(2, nv, 3, device=dev, dtype=torch.float64)
    out = torch.empty(nv, 3, device=dev)
    held = {}

    def keys_call():
        L.check(lib.cer_mesh_edge_keys_i64(p(fac, torch.int32), nf, nv, p(keys, torch.int64), st), "keys")

    def sort_call():
        held["sorted"] = torch.sort(keys).values

    def emit_call():
        s = held["sorted"]
        L.check(lib.cer_mesh_edge_count(p(s, torch.int64), nf, p(partials, torch.int32), p(offsets, torch.int64), p(totals, torch.int64), st), "count")
        assert int(totals[0].cpu()) == nn                    # the host read of the call
        L.check(lib.cer_mesh_edge_emit_i32(p(s, torch.int64), nf, p(offsets, torch.int64), nn, p(owner, torch.int32), p(e_nbrs, torch.int32),
                                           p(e_along, torch.int32), p(e_against, torch.int32), st), "emit")

    def starts_call():
        held["starts"] = torch.searchsorted(owner, torch.arange(nv + 1, device=dev, dtype=torch.int32)).to(torch.int32)

    def prepare_call():
        L.check(lib.cer_mesh_smooth_prepare_f32(p(ver), nv, p(starts, torch.int32), p(nbrs, torch.int32), p(along, torch.int32), p(against, torch.int32), nn,
                                                0, p(walk, torch.int32), p(flags, torch.uint8), p(state[0], torch.float64), st), "prepare")

    def step_call():
        L.check(lib.cer_mesh_smooth_steps_f64(p(state[0], torch.float64), p(state[1], torch.float64), nv, p(starts, torch.int32), p(walk, torch.int32), nn,
                                              p(flags, torch.uint8), 0.5, -0.53, 1, st), "step")

    def finish_call():
        L.check(lib.cer_mesh_smooth_finish_f32(p(state[1], torch.float64), p(ver), p(flags, torch.uint8), nv, p(out), st), "finish")

    def torch_edges_call():
        held["torch_edges"] = torch_edges(fac, nv)

    def torch_step_call():
        lo, hi = held["torch_edges"][0].long(), held["torch_edges"][1].long()
        held["torch_step"] = torch_step(state[0], lo, hi, 0.5)

    stages = (("edge_keys_ms", keys_call), ("edge_sort_ms", sort_call), ("edge_count_emit_ms", emit_call), ("nbr_starts_ms", starts_call),
              ("topology_report_ms", lambda: ME.mesh_topology(fac, nv)), ("smooth_prepare_ms", prepare_call), ("smooth_step_ms", step_call),
              ("smooth_finish_ms", finish_call), ("torch_edges_ms", torch_edges_call), ("torch_step_ms", torch_step_call))
    for _, fn in stages:                                     # warm-up, in order: every stage reads what the one before it wrote
        fn()
    torch.cuda.synchronize()
    rows = {k: [] for k, _ in stages}
    rows["mesh_edges_call_ms"], rows["taubin_10_call_ms"] = [], []
    for _ in range(args.rounds):
        for key, fn in stages:
            rows[key].append(timed(fn)[1])
        for key, fn in (("mesh_edges_call_ms", lambda: ME.mesh_edges(fac, nv)), ("taubin_10_call_ms", lambda: ME.smooth_mesh(ver, fac, 10))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            rows[key].append(1e3 * (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in rows.items()}
    # one step: starts, walk and flags read once, the source state read once (every row is somebody's neighbour, and its own), the target written
    step_bytes = (nv + 1) * 4 + nn * 4 + nv + 2 * nv * 24
    gathered_bytes = (nv + 1) * 4 + nn * 4 + nv + nn * 24 + 2 * nv * 24                      # what the lanes ask for: 24 bytes per list entry
    rate = step_bytes / (med["smooth_step_ms"] * 1e-3)
    table = ME.edge_table(starts, nbrs, along, against)
    t_edges = held["torch_edges"]
    lo, hi = table[0].long(), table[1].long()
    ours = state[1]                                          # the last step_call's result: all movable on a closed mesh, weight 0.5
    theirs = torch_step(state[0], lo, hi, 0.5)
    result = {"rounds": args.rounds, "device": torch.cuda.get_device_name(0), "height": H, "width": W, "views": len(SPHERE_DIRS),
              "grid": {"origin": list(grid.origin), "voxel": grid.voxel, "dims": list(grid.dims)}, "nv": nv, "nf": nf, "keys": 6 * nf, "nn": nn,
              "edges": nn // 2, "topology": report, "taubin_10_info": info, "distance_to_the_sphere": {"input": dist(ver), "taubin_10": dist(smoothed)},
              **med, "all_rounds": rows,
              "step": {"least_bytes": step_bytes, "bytes_the_lanes_ask_for": gathered_bytes, "least_bytes_per_second": rate, "hbm_peak_bytes_per_second": HBM_PEAK,
                       "fraction_of_hbm_peak": rate / HBM_PEAK, "asked_bytes_per_second": gathered_bytes / (med["smooth_step_ms"] * 1e-3)},
              "stages_equal_the_call": bool(torch.equal(held["starts"], starts) and torch.equal(e_nbrs, nbrs) and torch.equal(e_along, along)
                                            and torch.equal(e_against, against)),
              "torch_edge_table_equal": bool(all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(table, t_edges))),
              "torch_step_max_abs_difference": float((ours - theirs).abs().max()),
              "torch_edges_over_mesh_edges_call": med["torch_edges_ms"] / med["mesh_edges_call_ms"],
              "torch_step_over_step": med["torch_step_ms"] / med["smooth_step_ms"]}
    print(json.dumps({k: v for k, v in result.items() if k != "all_rounds"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
