"""Surface mesh at depth maps of 1600x1184, two scenes, grids at resolutions 256 and 512 each:

  scan    the synthetic 49-view scan: the depth maps of `synthetic_depth_maps`, fused by `fusion.fuse_depth_maps` (every view against its ring
          neighbours), the grid of `grid_for` around the central 99 % (per axis) of the fused cloud.  The scene is a plane, so the grid is a
          thin slab: a few hundred thousand nodes, 49 views each.
  sphere  ten analytic views of a unit sphere (tests/mesh_reference.py's case at full size), a cubic grid of resolution + 1 nodes per axis
          around it: 17 M and 135 M nodes, the size a volumetric user runs.

    python tools/bench_mesh.py [--views 49] [--size 1184x1600] [--neighbours 10] [--resolutions 256,512] [--rounds 3] [--out profiles/mesh_bench.json]

Between HIP events, medians of --rounds rounds after a warm-up: the four stages one by one through the C ABI - integrate, cells, count
(both compactions' count and scan), emit (vertices, then faces) - and `mesh_from_depth_maps` as a whole call on the host clock.  The plumbing
baseline is the integration restated in torch on the device (fp64, the contract's associations, z-slabs of --chunk nodes), interleaved with
the kernel round by round; its volume is compared with the kernel's bit for bit.  Needs a GPU."""
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

SPHERE_DIRS = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 1), (-1, 1, -1), (1, -1, -1), (-1, -1, 1))


def torch_tsdf(depths, masks, Ks, Es, grid, trunc, views, chunk):
    """the integration in torch ops on the device, fp64, slab by slab along z"""
    dev = depths.device
    N, h, w = depths.shape
    K, E = Ks.to(dev, torch.float64), Es.to(dev, torch.float64)
    (ox, oy, oz), voxel, (nx, ny, nz) = grid
    x = ox + torch.arange(nx, device=dev, dtype=torch.float64) * voxel
    y = oy + torch.arange(ny, device=dev, dtype=torch.float64) * voxel
    z = oz + torch.arange(nz, device=dev, dtype=torch.float64) * voxel
    tsdf = torch.empty(nz, ny, nx, device=dev, dtype=torch.float32)
    weight = torch.empty(nz, ny, nx, device=dev, dtype=torch.int32)
    slab = max(1, chunk // (nx * ny))
    for k0 in range(0, nz, slab):
        px, py, pz = torch.broadcast_tensors(x[None, None, :], y[None, :, None], z[k0:k0 + slab, None, None])
        total = torch.zeros(px.shape, device=dev, dtype=torch.float64)
        count = torch.zeros(px.shape, device=dev, dtype=torch.int32)
        for v in views:
            e, k = E[v], K[v]
            cx = ((e[0, 0] * px + e[0, 1] * py) + e[0, 2] * pz) + e[0, 3]
            cy = ((e[1, 0] * px + e[1, 1] * py) + e[1, 2] * pz) + e[1, 3]
            cz = ((e[2, 0] * px + e[2, 1] * py) + e[2, 2] * pz) + e[2, 3]
            ux = (k[0, 0] * cx + k[0, 1] * cy) + k[0, 2] * cz
            uy = (k[1, 0] * cx + k[1, 1] * cy) + k[1, 2] * cz
            uz = (k[2, 0] * cx + k[2, 1] * cy) + k[2, 2] * cz
            a, b = ux / uz + 0.5, uy / uz + 0.5
            ok = (uz > 0) & (a >= 0) & (a < w) & (b >= 0) & (b < h)
            xi = torch.where(ok, a.floor(), torch.zeros_like(a)).long()
            yi = torch.where(ok, b.floor(), torch.zeros_like(b)).long()
            ok &= masks[v][yi, xi] != 0
            d = depths[v][yi, xi].double()
            ok &= torch.isfinite(d) & (d > 0)
            sdf = d - uz
            ok &= sdf >= -trunc
            t = torch.where(sdf >= trunc, torch.ones_like(sdf), sdf / trunc)
            total = torch.where(ok, total + t, total)
            count += ok.int()
        tsdf[k0:k0 + slab] = torch.where(count > 0, total / count.double(), torch.ones_like(total)).float()
        weight[k0:k0 + slab] = count
    return tsdf, weight


def sphere_scene(H, W, dev, radius=1.0, dist=4.0):
    """ten analytic views of a unit sphere at the origin: z depth by ray-sphere intersection, mask = hit -> (depths, masks, Ks, Es), the maps
    on the device"""
    focal = 60.0 * W / 64.0
    K = torch.tensor([[focal, 0.0, (W - 1) / 2.0], [0.0, focal, (H - 1) / 2.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    v, u = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    rays = torch.stack([(u - K[0, 2]) / focal, (v - K[1, 2]) / focal, torch.ones_like(u)], -1)
    depths, masks, Es = [], [], []
    for d in SPHERE_DIRS:
        fwd = -np.asarray(d, np.float64) / np.linalg.norm(d)
        up = np.array([0.0, 0.0, 1.0]) if abs(fwd[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
        right = np.cross(up, fwd) / np.linalg.norm(np.cross(up, fwd))
        R = np.stack([right, np.cross(fwd, right), fwd])
        E = np.eye(4)
        E[:3, :3], E[:3, 3] = R, -R @ (-dist * fwd)
        c = torch.tensor(E[:3, 3], device=dev)               # the sphere's centre (the origin) in camera coordinates
        aa, bb = (rays * rays).sum(-1), rays @ c
        disc = bb * bb - aa * (float(c @ c) - radius * radius)
        hit = disc > 0
        depths.append(torch.where(hit, (bb - disc.clamp_min(0).sqrt()) / aa, torch.zeros_like(aa)).float())
        masks.append(hit.to(torch.uint8))
        Es.append(torch.from_numpy(E).float())
    return torch.stack(depths), torch.stack(masks), K.float()[None].repeat(len(SPHERE_DIRS), 1, 1), torch.stack(Es)


def measure(est, masks, Ks, Es, refs, grid, args):
    """one grid: the four stages between events, the torch restatement of the first interleaved, the whole call on the host clock"""
    from cer_mvs_amd import _lib as L
    from cer_mvs_amd import mesh as ME
    lib, dev = L.load(), est.device
    N, H, W = (int(v) for v in est.shape)
    cams = ME.forward_cams(Ks, Es).to(dev)
    vlist = torch.tensor(refs, dtype=torch.int32, device=dev)
    origin, voxel, (nx, ny, nz) = ME._grid(grid, "bench_mesh")
    trunc = 3.0 * voxel
    nodes = nx * ny * nz
    tsdf = torch.empty(nz, ny, nx, device=dev)
    weight = torch.empty(nz, ny, nx, device=dev, dtype=torch.int32)
    cells = torch.empty(nz - 1, ny - 1, nx - 1, device=dev, dtype=torch.int16)
    P = int(lib.cer_mesh_partials(nx, ny, nz))
    partials = torch.empty(P, device=dev, dtype=torch.int32)
    offsets = torch.empty(P + 2, device=dev, dtype=torch.int64)
    totals = torch.zeros(2, device=dev, dtype=torch.int64)
    vmap = torch.empty(nodes * 8, device=dev, dtype=torch.int32)
    p = lambda t, dt=torch.float32: L.dev_ptr(t, "t", dt)
    st = L.cur_stream()

    def integrate():
        L.check(lib.cer_tsdf_integrate_f32(p(est), p(masks, torch.uint8), p(cams, torch.float64), N, H, W, p(vlist, torch.int32), len(refs), origin,
                                           voxel, nx, ny, nz, trunc, p(tsdf), p(weight, torch.int32), st), "integrate")

    def cell_pass():
        L.check(lib.cer_mesh_cells_u16(p(tsdf), p(weight, torch.int32), nx, ny, nz, 1, p(cells, torch.int16), st), "cells")

    def count():
        L.check(lib.cer_mesh_count(p(cells, torch.int16), nx, ny, nz, p(partials, torch.int32), p(offsets, torch.int64), p(totals, torch.int64), st), "count")
    integrate(), cell_pass(), count()
    nv, nf = (int(v) for v in totals.cpu())
    vert = torch.empty(nv, 3, device=dev)
    face = torch.empty(nf, 3, device=dev, dtype=torch.int32)

    def emit():
        L.check(lib.cer_mesh_emit_f32(p(tsdf), p(cells, torch.int16), origin, voxel, nx, ny, nz, p(offsets, torch.int64), nv, nf, nv, nf,
                                      p(vmap, torch.int32), p(vert) if nv else None, p(face, torch.int32) if nf else None, st), "emit")
    emit()
    whole = lambda: ME.mesh_from_depth_maps(est, masks, Ks, Es, grid, views=refs)
    base = lambda: torch_tsdf(est, masks, Ks, Es, grid, trunc, refs, args.chunk)
    whole(), base()
    torch.cuda.synchronize()
    rows = {k: [] for k in ("integrate_ms", "cells_ms", "count_ms", "emit_ms", "torch_integrate_ms", "mesh_from_depth_maps_ms")}
    for _ in range(args.rounds):
        for key, fn in (("integrate_ms", integrate), ("torch_integrate_ms", base), ("cells_ms", cell_pass), ("count_ms", count), ("emit_ms", emit)):
            out, ms = timed(fn)
            rows[key].append(ms)
            if key == "torch_integrate_ms":
                bt, bw = out
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        whole()
        torch.cuda.synchronize()
        rows["mesh_from_depth_maps_ms"].append(1e3 * (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in rows.items()}
    entry = {"grid": {"origin": list(grid.origin), "voxel": grid.voxel, "dims": list(grid.dims)}, "nodes": nodes, "views": len(refs), "trunc": trunc,
             "nv": nv, "nf": nf, "observed": int((weight >= 1).sum()), "all_rounds": rows, **med,
             "torch_over_kernel": med["torch_integrate_ms"] / med["integrate_ms"],
             "integrate_node_views_per_s": nodes * len(refs) / (med["integrate_ms"] * 1e-3),
             "torch_weight_equal": bool(torch.equal(bw, weight)),
             "torch_tsdf_bits_equal": bool(torch.equal(bt.view(torch.int32), tsdf.view(torch.int32))),
             "workspace_bytes": {"volumes": nodes * 8, "cells": int(cells.numel()) * 2, "vmap": nodes * 32}}
    print(json.dumps({k: v for k, v in entry.items() if k != "all_rounds"}), flush=True)
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--size", default="1184x1600", help="HxW of the depth maps")
    ap.add_argument("--neighbours", type=int, default=10)
    ap.add_argument("--resolutions", default="256,512")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1 << 22, help="nodes per slab of the torch restatement")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh: needs a GPU")
    dev = torch.device("cuda:0")
    from cer_mvs_amd import fusion, mesh as ME
    from cer_mvs_amd.synthetic import synthetic_depth_maps, synthetic_scene

    H, W = (int(v) for v in args.size.lower().split("x"))
    N, nb = args.views, args.neighbours
    resolutions = [int(r) for r in args.resolutions.split(",")]
    result = {"height": H, "width": W, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "scan": {}, "sphere": {}}

    # ---- the sphere: a cubic grid of resolution + 1 nodes per axis over [-1.2, 1.2]^3
    depths, masks, Ks, Es = sphere_scene(H, W, dev)
    result["sphere"] = {"views": len(SPHERE_DIRS), "mask_area": float(masks.float().mean()), "resolutions": {}}
    for res in resolutions:
        voxel = 2.4 / res
        grid = ME.Grid((-1.2 + 0.013 * voxel,) * 3, voxel, (res + 1,) * 3)
        result["sphere"]["resolutions"][str(res)] = measure(depths, masks, Ks, Es, list(range(len(SPHERE_DIRS))), grid, args)
        torch.cuda.empty_cache()
    del depths, masks

    # ---- the scan
    t0 = time.perf_counter()
    _, poses, intr, _ = synthetic_scene(32, 32, N - 1, seed=1)
    Ks, Es = intr[0].clone().float(), poses[0].float()
    Ks[:, 0, 0] = Ks[:, 1, 1] = 1.8 * W
    Ks[:, 0, 2], Ks[:, 1, 2] = W / 2.0, H / 2.0
    depths = synthetic_depth_maps(H, W, N - 1, seed=1).to(dev)
    print(f"depth maps: {N} views of {W}x{H} in {time.perf_counter() - t0:.1f} s", flush=True)
    pairs = [(i, p[:nb]) for i, p in enumerate(ring_pairs(N, nb))]
    masks, est, thre, hist = fusion.fuse_depth_maps(depths, Ks, Es, pairs, glb=0.25)
    refs = list(range(N))
    xyz, _ = fusion.point_cloud(masks, est, Ks, Es, torch.zeros(N, 3, H, W, device=dev), refs)
    # the bisection holds the mean mask area at glb whatever the views agree on, so the steep views of the ring leave points far off the
    # plane: the grid goes around the central 99 % of every axis (quantiles of a subsample of about a million points)
    sub = xyz[::max(1, len(xyz) >> 20)].double()
    q = torch.quantile(sub, torch.tensor([0.005, 0.995], device=dev, dtype=torch.float64), dim=0)
    core = xyz[((xyz >= q[0].float()) & (xyz <= q[1].float())).all(1)]
    print(f"fused: mean mask area {hist[-1][1]:.4f}, {len(xyz)} points, {len(core)} in the central box", flush=True)
    result["scan"] = {"views": N, "neighbours": nb, "points": int(len(xyz)), "points_in_central_box": int(len(core)), "mean_mask_area": hist[-1][1],
                      "resolutions": {}}
    for res in resolutions:
        grid = ME.grid_for(core, resolution=res, max_nodes=2 ** 30)
        result["scan"]["resolutions"][str(res)] = measure(est, masks, Ks, Es, refs, grid, args)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
