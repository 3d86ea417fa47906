"""Mesh hole filling on the 513^3 sphere case of tools/bench_mesh.py: ten analytic views of a unit sphere at 1600x1184, the
mesh of `mesh_from_depth_maps` on a cubic grid of --resolution + 1 nodes per axis (2.58 M vertices and 5.15 M faces at 512), open where the
views leave nodes unobserved.

    python tools/bench_mesh_fill.py [--size 1184x1600] [--resolution 512] [--rounds 3] [--max-edges 16,64,1024] [--out profiles/mesh_fill_bench.json]

Per `max_edges`, between HIP events, medians of --rounds interleaved rounds after a warm-up: `mesh_edges` (shared by every value), the
successor kernel, the heads kernel, the torch plumbing between them and the fill (`nonzero`, the two exclusive sums and the host read of
the totals), and the fill kernel with the copies of the input rows; and `fill_holes` as a whole call on the host clock.  Beside the times:
the number of holes, the longest walk of the heads kernel (the most steps one thread takes, counted on the host from the successor table),
the loops before and after from `mesh_topology`, and whether the stages' outputs equal the call's.  Needs a GPU."""
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
from bench_mesh import SPHERE_DIRS, sphere_scene  # noqa: E402


def walks(nxt, max_edges):
    """the steps the heads kernel takes per vertex with a successor (the contract's stopping rules, finite vertices): numpy, one step of all
    walks at a time -> (longest, mean, walkers)"""
    nv = len(nxt)
    start = np.flatnonzero(nxt >= 0)
    cur, steps, live = nxt[start].astype(np.int64), np.ones(len(start), np.int64), np.ones(len(start), bool)
    while live.any():
        i = np.flatnonzero(live)
        u = cur[i]
        stop = (u == start[i]) | (u < 0) | (u >= nv) | (u < start[i]) | (steps[i] >= max_edges)
        live[i[stop]] = False
        go = i[~stop]
        cur[go] = nxt[cur[go]]
        steps[go] += 1
    return (int(steps.max()), float(steps.mean()), len(start)) if len(start) else (0, 0.0, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1184x1600", help="HxW of the sphere's depth maps")
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-edges", default="16,64,1024")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_fill_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_fill: needs a GPU")
    dev = torch.device("cuda:0")
    from cer_mvs_amd import _lib as L
    from cer_mvs_amd import mesh as ME

    H, W = (int(v) for v in args.size.lower().split("x"))
    res = args.resolution
    limits = [int(v) for v in args.max_edges.split(",")]
    depths, masks, Ks, Es = sphere_scene(H, W, dev)
    voxel = 2.4 / res
    grid = ME.Grid((-1.2 + 0.013 * voxel,) * 3, voxel, (res + 1,) * 3)
    ver, fac = ME.mesh_from_depth_maps(depths, masks, Ks, Es, grid, trunc=3.0 * voxel)
    del depths, masks
    torch.cuda.empty_cache()
    lib, st = L.load(), L.cur_stream()
    nv, nf = int(ver.shape[0]), int(fac.shape[0])
    p = lambda t, dt=torch.float32: L.dev_ptr(t, "t", dt)
    before = ME.mesh_topology(fac, nv)
    print(f"{nv} vertices, {nf} faces; {before}", flush=True)

    starts, nbrs, along, against = ME.mesh_edges(fac, nv)
    nn = int(nbrs.shape[0])
    nxt = torch.empty(nv, device=dev, dtype=torch.int32)
    length = torch.empty(nv, device=dev, dtype=torch.int32)
    held = {}

    def next_call():
        L.check(lib.cer_mesh_hole_next_i32(p(starts, torch.int32), p(nbrs, torch.int32), p(along, torch.int32), p(against, torch.int32), nv, nn,
                                           p(nxt, torch.int32), st), "next")

    def heads_call(limit):
        L.check(lib.cer_mesh_hole_heads_i32(p(nxt, torch.int32), p(ver), nv, limit, p(length, torch.int32), st), "heads")

    def offsets_call():
        heads = torch.nonzero(length).reshape(-1)
        lens = length[heads]
        n_faces = torch.where(lens == 3, torch.ones_like(lens), lens).long()
        n_vertices = (lens > 3).long()
        fo, vo = (torch.cumsum(n_faces, 0) - n_faces).contiguous(), (torch.cumsum(n_vertices, 0) - n_vertices).contiguous()
        af, av = (int(x) for x in torch.stack([n_faces.sum(), n_vertices.sum()]).cpu().tolist())       # the host read of the call
        held.update(heads=heads.to(torch.int32), lens=lens.contiguous(), fo=fo, vo=vo, af=af, av=av)

    def fill_call():
        h, af, av = held["heads"], held["af"], held["av"]
        out_v = torch.empty(nv + av, 3, device=dev)
        out_f = torch.empty(nf + af, 3, device=dev, dtype=torch.int32)
        hole = torch.empty(nf + af, device=dev, dtype=torch.int32)
        out_v[:nv] = ver
        out_f[:nf] = fac
        hole[:nf] = -1
        L.check(lib.cer_mesh_hole_fill_f32(p(nxt, torch.int32), p(h, torch.int32), p(held["lens"], torch.int32), p(held["fo"], torch.int64),
                                           p(held["vo"], torch.int64), int(h.shape[0]), p(ver) if av else None, None, nv, nf, av, af,
                                           p(out_v) if av else None, p(out_f, torch.int32), p(hole, torch.int32), None, st), "fill")
        held.update(out=(out_v, out_f, hole))

    def kernel_only():
        h, af, av = held["heads"], held["af"], held["av"]
        out_v, out_f, hole = held["out"]
        L.check(lib.cer_mesh_hole_fill_f32(p(nxt, torch.int32), p(h, torch.int32), p(held["lens"], torch.int32), p(held["fo"], torch.int64),
                                           p(held["vo"], torch.int64), int(h.shape[0]), p(ver) if av else None, None, nv, nf, av, af,
                                           p(out_v) if av else None, p(out_f, torch.int32), p(hole, torch.int32), None, st), "fill")

    def stages(limit):
        return (("edges_ms", lambda: ME.mesh_edges(fac, nv)), ("next_ms", next_call), ("heads_ms", lambda: heads_call(limit)),
                ("offsets_ms", offsets_call), ("fill_with_copies_ms", fill_call), ("fill_kernel_ms", kernel_only))

    for limit in limits:                                     # warm-up, in order: every stage reads what the one before it wrote
        for _, fn in stages(limit):
            fn()
        ME.fill_holes(ver, fac, limit)
    torch.cuda.synchronize()
    rows = {limit: {k: [] for k, _ in stages(limit)} for limit in limits}
    for _ in range(args.rounds):                             # interleaved: every value in every round
        for limit in limits:
            for key, fn in stages(limit):
                rows[limit][key].append(timed(fn)[1])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ME.fill_holes(ver, fac, limit)
            torch.cuda.synchronize()
            rows[limit].setdefault("fill_holes_call_ms", []).append(1e3 * (time.perf_counter() - t0))
    table = nxt.cpu().numpy()
    per_limit = {}
    for limit in limits:
        for _, fn in stages(limit):
            fn()
        info = {}
        ov, of, hole, _ = ME.fill_holes(ver, fac, limit, info=info)
        sv, sf, sh = held["out"]
        after = ME.mesh_topology(of, int(ov.shape[0]))
        longest, mean, walkers = walks(table, limit)
        lens = held["lens"]
        per_limit[str(limit)] = {**{k: statistics.median(v) for k, v in rows[limit].items()}, "all_rounds": rows[limit], "info": info,
                                 "holes": info["holes"], "longest_hole": int(lens.max()) if lens.numel() else 0,
                                 "longest_walk_steps": longest, "mean_walk_steps": mean, "walking_threads": walkers,
                                 "boundary_loops_after": after["boundary_loops"], "boundary_edges_after": after["boundary_edges"],
                                 "oriented_after": after["oriented"], "edge_manifold_after": after["edge_manifold"],
                                 "stages_equal_the_call": bool(torch.equal(sv, ov) and torch.equal(sf, of) and torch.equal(sh, hole))}
        print(json.dumps({limit: {k: v for k, v in per_limit[str(limit)].items() if k != "all_rounds"}}), flush=True)
    result = {"rounds": args.rounds, "device": torch.cuda.get_device_name(0), "height": H, "width": W, "views": len(SPHERE_DIRS),
              "grid": {"origin": list(grid.origin), "voxel": grid.voxel, "dims": list(grid.dims)}, "nv": nv, "nf": nf, "nn": nn,
              "topology_before": before, "pinched_vertices": int((nxt == -2).sum()), "vertices_with_a_successor": int((nxt >= 0).sum()),
              "max_edges": per_limit}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
