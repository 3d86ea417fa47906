"""Exact point-to-mesh distance on the 513^3 sphere case of tools/bench_mesh.py: ten analytic views of a unit sphere at
1600x1184, the mesh of `mesh_from_depth_maps` on a cubic grid of --resolution + 1 nodes per axis (2.58 M vertices and 5.15 M faces at 512).

    python tools/bench_mesh_dist.py [--size 1184x1600] [--resolution 512] [--rounds 3] [--queries 1000000] [--max-dist-voxels 4]
                                    [--brute-queries 32] [--out profiles/mesh_dist_bench.json]

Two query sets of --queries points each: "near" - `sample_mesh` points moved along their face's normal by a normal deviate of one voxel -
and "box" - uniform in the grid's box, where most queries find nothing within the cut-off and pay for the whole walk.  Medians of --rounds
interleaved rounds after a warm-up, between HIP events unless said otherwise: the index build by stage (events inside `MeshIndex`), the
search on both sets with `sort_queries` on and off (the query sort is inside the timed call), the cell sweep - the default's
DEFAULT_CELL_EDGES * sqrt(area / faces with weight) at edge factors 1 .. 8 of the mean face's edge, build and both searches at each -
`evaluate_mesh` exact against sampled as whole calls on the host clock (spacing two voxels, the "near" set as ground truth), and the same
contract in torch ops on the device as a brute force over all faces, measured on --brute-queries queries and EXTRAPOLATED linearly to
--queries (its distances are compared with the kernel's on those queries).  Needs a GPU."""
import argparse
import json
import math
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from bench_cloud_eval import timed  # noqa: E402
from bench_mesh import SPHERE_DIRS, sphere_scene  # noqa: E402

SWEEP = (1.0, 2.0, 4.0, 8.0)


def torch_dist2(a, b, c, p):
    """cer_mvs.h's "Mesh distance" in torch ops, the select form: a, b, c float64 [nf, 3], p float64 [k, 1, 3] -> dist2 [k, nf]"""
    def dot(x, y):
        return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    r1 = (d1 <= 0) & (d2 <= 0)
    r2 = ~r1 & (d3 >= 0) & (d4 <= d3)
    r3 = ~r1 & ~r2 & (vc <= 0) & (d1 >= 0) & (d3 <= 0)
    r4 = ~r1 & ~r2 & ~r3 & (d6 >= 0) & (d5 <= d6)
    r5 = ~r1 & ~r2 & ~r3 & ~r4 & (vb <= 0) & (d2 >= 0) & (d6 <= 0)
    r6 = ~r1 & ~r2 & ~r3 & ~r4 & ~r5 & (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)
    w6 = (d4 - d3) / ((d4 - d3) + (d5 - d6))
    den = (va + vb) + vc
    zero = torch.zeros_like(d1)
    v = torch.where(r3, d1 / (d1 - d3), torch.where(r5, zero, torch.where(r6, 1.0 - w6, vb / den)))
    w = torch.where(r3, zero, torch.where(r5, d2 / (d2 - d6), torch.where(r6, w6, vc / den)))
    e = (a + v[..., None] * ab) + w[..., None] * ac
    q = torch.where(r1[..., None], a, torch.where(r2[..., None], b, torch.where(r4[..., None], c, e)))
    r = q - p
    return (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1184x1600", help="HxW of the sphere's depth maps")
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--queries", type=int, default=1000000)
    ap.add_argument("--max-dist-voxels", type=float, default=4.0, help="the cut-off, in voxels of the grid")
    ap.add_argument("--brute-queries", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_dist_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_dist: needs a GPU")
    dev = torch.device("cuda:0")
    from cer_mvs_amd import mesh as ME

    H, Wd = (int(v) for v in args.size.lower().split("x"))
    res, m = args.resolution, args.queries
    depths, masks, Ks, Es = sphere_scene(H, Wd, dev)
    voxel = 2.4 / res
    grid = ME.Grid((-1.2 + 0.013 * voxel,) * 3, voxel, (res + 1,) * 3)
    ver, fac = ME.mesh_from_depth_maps(depths, masks, Ks, Es, grid, trunc=3.0 * voxel)
    del depths, masks
    torch.cuda.empty_cache()
    nv, nf = int(ver.shape[0]), int(fac.shape[0])
    max_dist = float(torch.tensor(args.max_dist_voxels * voxel, dtype=torch.float32))
    _, W, shift, with_weight = ME._sample_table(ver, fac, nv, nf)
    area = math.ldexp(float(W), -shift)
    edge = math.sqrt(area / with_weight)
    gen = torch.Generator(dev).manual_seed(1)
    pts, _, nrm, _, _ = ME.sample_mesh(ver, fac, n=m, seed=5, normals=True)
    near = (pts + nrm * (voxel * torch.randn(m, 1, device=dev, generator=gen))).contiguous()
    box = ((torch.rand(m, 3, device=dev, generator=gen) * 2.4 - 1.2).float()).contiguous()
    del pts, nrm
    print(f"{nv} vertices, {nf} faces; area {area:.6f}, mean face edge sqrt(area / faces) {edge:.6f} ({edge / voxel:.3f} voxels), max_dist {max_dist:.6f}", flush=True)

    def build(cell=None, stages=None):
        return ME.MeshIndex(ver, fac, cell, max_dist, _stages=stages)

    def whole(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, 1e3 * (time.perf_counter() - t0)

    sets = {"near": near, "box": box}
    index = build()
    for q in sets.values():                                  # warm-up
        index.nearest(q, max_dist)
        index.nearest(q, max_dist, sort_queries=False)
    spacing = 2.0 * voxel
    ME.evaluate_mesh(ver, fac, near, spacing, max_dist=max_dist, tau=voxel)
    ME.evaluate_mesh(ver, fac, near, spacing, max_dist=max_dist, tau=voxel, method="exact")
    rows = {}
    for _ in range(args.rounds):                             # interleaved: every path in every round
        stages = []
        _, total = timed(lambda: build(stages=stages))
        rows.setdefault("build_ms", []).append(total)
        for (_, e0), (name, e1) in zip(stages, stages[1:]):
            rows.setdefault(f"build_{name}_ms", []).append(e0.elapsed_time(e1))
        for name, q in sets.items():
            rows.setdefault(f"nearest_{name}_ms", []).append(timed(lambda: index.nearest(q, max_dist))[1])
            rows.setdefault(f"nearest_{name}_closest_ms", []).append(timed(lambda: index.nearest(q, max_dist, closest=True))[1])
            rows.setdefault(f"nearest_{name}_unsorted_ms", []).append(timed(lambda: index.nearest(q, max_dist, sort_queries=False))[1])
            rows.setdefault(f"query_order_{name}_ms", []).append(timed(lambda: index._walk_order(q, m))[1])
        for factor in SWEEP:
            swept = build(factor * edge)
            rows.setdefault(f"sweep_{factor}_build_ms", []).append(timed(lambda: build(factor * edge))[1])
            for name, q in sets.items():
                rows.setdefault(f"sweep_{factor}_nearest_{name}_ms", []).append(timed(lambda: swept.nearest(q, max_dist))[1])
            del swept
        rows.setdefault("evaluate_samples_call_ms", []).append(whole(lambda: ME.evaluate_mesh(ver, fac, near, spacing, max_dist=max_dist, tau=voxel))[1])
        rows.setdefault("evaluate_exact_call_ms", []).append(
            whole(lambda: ME.evaluate_mesh(ver, fac, near, spacing, max_dist=max_dist, tau=voxel, method="exact"))[1])
    med = {k: statistics.median(v) for k, v in rows.items()}
    sweep = {}
    for factor in SWEEP:
        swept = build(factor * edge)
        info = swept.info()
        sweep[str(factor)] = dict(info, pairs_per_face=info["pairs"] / max(info["faces_indexed"], 1), pairs_per_cell=info["pairs"] / max(info["cells"], 1),
                                  build_ms=med[f"sweep_{factor}_build_ms"], nearest_near_ms=med[f"sweep_{factor}_nearest_near_ms"],
                                  nearest_box_ms=med[f"sweep_{factor}_nearest_box_ms"])
        del swept
    # the figures of the default index, and what the searches found
    info = index.info()
    found = {name: int((index.nearest(q, max_dist)[1] >= 0).sum()) for name, q in sets.items()}
    metrics = {"samples": ME.evaluate_mesh(ver, fac, near, spacing, max_dist=max_dist, tau=voxel),
               "exact": ME.evaluate_mesh(ver, fac, near, spacing, max_dist=max_dist, tau=voxel, method="exact")}
    # the brute force in torch ops, fp64, every face for every query: a few queries at a time, extrapolated
    k = args.brute_queries
    sub = near[:k].double()
    a, b, c = (ver.double().index_select(0, fac[:, i].long()) for i in range(3))
    limit = max_dist * max_dist

    def brute():
        out = []
        for s in range(0, k, 4):
            d2 = torch_dist2(a, b, c, sub[s:s + 4, None, :])
            d2 = torch.where(d2 <= limit, d2, torch.full_like(d2, math.inf))
            out.append(d2.min(1).values)
        return torch.cat(out)
    brute()
    brute_ms = [timed(brute)[1] for _ in range(args.rounds)]
    want = torch.where(torch.isinf(brute()), torch.full((k,), math.inf, device=dev), brute().sqrt().float())
    got = index.nearest(near[:k].contiguous(), max_dist)[0]
    brute_same = bool(torch.equal(got.view(torch.int32), want.view(torch.int32)))
    result = {"rounds": args.rounds, "device": torch.cuda.get_device_name(0), "height": H, "width": Wd, "views": len(SPHERE_DIRS),
              "grid": {"origin": list(grid.origin), "voxel": grid.voxel, "dims": list(grid.dims)}, "nv": nv, "nf": nf, "area": area,
              "faces_with_weight": with_weight, "mean_face_edge": edge, "queries": m, "max_dist": max_dist, "max_dist_voxels": args.max_dist_voxels,
              "index": dict(info, pairs_per_face=info["pairs"] / max(info["faces_indexed"], 1), pairs_per_cell=info["pairs"] / max(info["cells"], 1),
                            bytes=48 * nf + 4 * info["pairs"] + 16 * info["cells"] + 8),
              "found": found, "medians_ms": med, "all_rounds_ms": rows, "cell_sweep_edge_factors": sweep, "default_edge_factor": ME.DEFAULT_CELL_EDGES,
              "queries_per_s": {name: m / (1e-3 * med[f"nearest_{name}_ms"]) for name in sets},
              "evaluate": {"spacing": spacing, "tau": voxel, "metrics": metrics},
              "torch_brute_force": {"queries": k, "ms": statistics.median(brute_ms), "extrapolated_to_queries_ms": statistics.median(brute_ms) * m / k,
                                    "extrapolated": True, "same_distances_as_the_kernel": brute_same}}
    print(json.dumps({k2: v for k2, v in result.items() if k2 != "all_rounds_ms"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
