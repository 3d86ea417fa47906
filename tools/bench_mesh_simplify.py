"""Mesh simplification by vertex clustering on the 513^3 sphere case of tools/bench_mesh.py: ten analytic views of a unit
sphere at 1600x1184, the mesh of `mesh_from_depth_maps` on a cubic grid of --resolution + 1 nodes per axis (2.58 M vertices and 5.15 M faces
at 512), simplified at cells of --voxels mesh voxels (default 2 and 4) with both representatives.

    python tools/bench_mesh_simplify.py [--size 1184x1600] [--resolution 512] [--voxels 2,4] [--rounds 3] [--out profiles/mesh_simplify_bench.json]

Between HIP events, medians of --rounds rounds after a warm-up, stage by stage as `simplify_vertex_clustering` runs them: the index build
(`cloud_eval.CloudIndex`: keys, stable sort, cell table, with its two host reads), the corner list of the input (`vertex_faces`, which the
quadric form walks), the cluster map, the representatives, the face remap, the two stable sorts, the heads and the selection (`_select`
with the corner list of the triples, and the inverse cluster map); and the whole call on the host clock.  Beside them, interleaved round by
round, the same contract restated in torch ops on the device (`torch.unique`, `index_add_`, `torch.linalg.solve`, `torch.unique(dim=0)`): its
time only - its sums are atomic, so its bits differ from run to run - with its faces compared exactly and its positions by their largest
difference.  Output sizes and the distance of the output vertices to the unit sphere are reported for every case.  Needs a GPU."""
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

KEY_MASK = (1 << 21) - 1


def torch_simplify(ver, fac, cell, quadric, regularisation=1e-3):
    """the contract in torch ops on the device (finite vertices only): (vertices', faces', cluster)"""
    v = ver.double()
    origin = v.amin(0)
    c = torch.floor((v - origin) / cell).long()
    uniq, inv = torch.unique((c[:, 2] << 42) | (c[:, 1] << 21) | c[:, 0], return_inverse=True)
    nc = int(uniq.shape[0])
    count = torch.bincount(inv, minlength=nc)
    mean = torch.zeros(nc, 3, device=v.device, dtype=torch.float64).index_add_(0, inv, v) / count[:, None].double()
    f = fac.long()
    rep = mean
    if quadric:
        cells = torch.stack([uniq & KEY_MASK, (uniq >> 21) & KEY_MASK, uniq >> 42], 1).double()
        base = origin + (cells + 0.5) * cell
        A, B, C = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        n = torch.linalg.cross(B - A, C - A)
        outer = (n[:, :, None] * n[:, None, :]).reshape(-1, 9)
        M = torch.zeros(nc, 9, device=v.device, dtype=torch.float64)
        q = torch.zeros(nc, 3, device=v.device, dtype=torch.float64)
        for k in range(3):                                   # a face is visited once per corner: the sum of vertex quadrics
            owner = inv[f[:, k]]
            d = (n * (A - base[owner])).sum(1)
            M.index_add_(0, owner, outer)
            q.index_add_(0, owner, n * d[:, None])
        M = M.reshape(nc, 3, 3)
        lam = regularisation * (M[:, 0, 0] + M[:, 1, 1] + M[:, 2, 2]) / 3.0
        safe = lam > 0.0
        mat = M + torch.where(safe, lam, torch.ones_like(lam))[:, None, None] * torch.eye(3, device=v.device, dtype=torch.float64)
        x = torch.linalg.solve(mat, (q + lam[:, None] * (mean - base))[:, :, None])[:, :, 0]
        ok = safe & torch.isfinite(x).all(1) & (x.abs() <= cell / 2.0).all(1)
        rep = torch.where(ok[:, None], base + x, mean)
    t = inv[f]
    valid = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    first = t.argmin(1)
    t = torch.gather(t, 1, (first[:, None] + torch.arange(3, device=v.device)) % 3)
    where = torch.nonzero(valid).reshape(-1)
    _, which = torch.unique(t[where], dim=0, return_inverse=True)
    head = torch.full((int(which.max()) + 1 if which.numel() else 0,), f.shape[0], device=v.device, dtype=torch.int64)
    head.scatter_reduce_(0, which, where, "amin")
    kept = t[torch.sort(head).values]
    used = torch.zeros(nc, device=v.device, dtype=torch.bool)
    used[kept.reshape(-1)] = True
    new = torch.cumsum(used, 0) - 1
    cluster = torch.where(used[inv], new[inv], torch.full_like(inv, -1)).to(torch.int32)
    return rep.float()[used], new[kept].to(torch.int32), cluster


def sphere_distance(vertices):
    d = (vertices.double().norm(dim=1) - 1.0).abs()
    return {"mean": float(d.mean()), "max": float(d.max())}


def measure(ver, fac, cell, representative, args):
    from cer_mvs_amd import _lib as L
    from cer_mvs_amd import mesh as ME
    from cer_mvs_amd.cloud_eval import CloudIndex
    lib, dev = L.load(), ver.device
    nv, nf = int(ver.shape[0]), int(fac.shape[0])
    quadric = representative == "quadric"
    p = lambda t, dt=torch.float32: L.dev_ptr(t, "t", dt)
    st = L.cur_stream()
    info = {}
    out_v, out_f, out_cluster, _ = ME.simplify_vertex_clustering(ver, fac, cell, representative=representative, info=info)
    print(f"cell {cell:.6f} ({representative}): {nv} -> {out_v.shape[0]} vertices, {nf} -> {out_f.shape[0]} faces, {info}", flush=True)
    starts, corner_order = ME.vertex_faces(fac, nv)
    index = CloudIndex(ver, cell)
    nc = int(index.cells)
    cluster = torch.empty(nv, device=dev, dtype=torch.int32)
    reps = torch.empty(nc, 3, device=dev)
    took = torch.zeros(nc, device=dev, dtype=torch.uint8)
    triples = torch.empty(nf, 3, device=dev, dtype=torch.int32)
    valid = torch.empty(nf, device=dev, dtype=torch.uint8)
    keep = torch.empty(nf, device=dev, dtype=torch.uint8)
    state = {}

    def map_call():
        L.check(lib.cer_mesh_cluster_map_i32(p(index.order, torch.int64), p(index.cell_start, torch.int64), nv, nc, p(cluster, torch.int32), st), "map")

    def reps_call():
        L.check(lib.cer_mesh_cluster_reps_f32(p(ver), nv, p(fac, torch.int32), nf, p(starts, torch.int32), p(corner_order, torch.int32),
                                              p(index.order, torch.int64), p(index.cell_start, torch.int64), p(index.cell_keys, torch.int64), nc,
                                              index.origin, cell, int(quadric), 1e-3, None, p(reps), None, p(took, torch.uint8), st), "reps")

    def faces_call():
        L.check(lib.cer_mesh_cluster_faces_i32(p(fac, torch.int32), nf, p(cluster, torch.int32), nv, p(triples, torch.int32), p(valid, torch.uint8), st),
                "faces")

    def sorts():
        t = triples.long()
        by_bc = torch.sort((t[:, 1] << 31) | t[:, 2], stable=True).indices
        state["perm"] = by_bc[torch.sort(t[:, 0][by_bc], stable=True).indices].contiguous()

    def heads_call():
        L.check(lib.cer_mesh_face_heads_u8(p(triples, torch.int32), p(valid, torch.uint8), p(state["perm"], torch.int64), nf, p(keep, torch.uint8), st),
                "heads")

    def selection():
        t_starts, t_order = ME._corner_list(triples.reshape(-1), nc)
        sv, sf, kept, _, _ = ME._select(reps, triples, keep, t_starts, t_order, None, None)
        new_of = torch.full((nc + 1,), -1, device=dev, dtype=torch.int32)
        new_of[kept.long()] = torch.arange(int(sv.shape[0]), device=dev, dtype=torch.int32)
        return sv, sf, new_of[cluster.long()]
    stages = (("index_build_ms", lambda: CloudIndex(ver, cell)), ("input_corner_list_ms", lambda: ME.vertex_faces(fac, nv)), ("cluster_map_ms", map_call),
              ("representatives_ms", reps_call), ("face_remap_ms", faces_call), ("two_sorts_ms", sorts), ("face_heads_ms", heads_call),
              ("selection_ms", selection), ("torch_ops_ms", lambda: torch_simplify(ver, fac, cell, quadric)))
    for _, fn in stages:                                     # warm-up, in order: every stage reads what the one before it wrote
        staged = fn()
    torch.cuda.synchronize()
    rows = {k: [] for k, _ in stages}
    rows["whole_call_ms"] = []
    for _ in range(args.rounds):
        for key, fn in stages:
            out, ms = timed(fn)
            rows[key].append(ms)
            if key == "selection_ms":
                staged = out
            if key == "torch_ops_ms":
                tv, tf, tc = out
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ME.simplify_vertex_clustering(ver, fac, cell, representative=representative)
        torch.cuda.synchronize()
        rows["whole_call_ms"].append(1e3 * (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in rows.items()}
    kernels = ("cluster_map_ms", "representatives_ms", "face_remap_ms", "face_heads_ms")
    same_shape = tv.shape == out_v.shape
    entry = {"cell": cell, "representative": representative, "nv": nv, "nf": nf, "out_vertices": int(out_v.shape[0]), "out_faces": int(out_f.shape[0]), **info,
             "distance_to_the_sphere": sphere_distance(out_v), "input_distance_to_the_sphere": sphere_distance(ver), **med,
             "new_kernels_ms": sum(med[k] for k in kernels), "torch_ops_over_whole_call": med["torch_ops_ms"] / med["whole_call_ms"], "all_rounds": rows,
             "stages_equal_the_call": bool(torch.equal(staged[0].view(torch.int32), out_v.view(torch.int32)) and torch.equal(staged[1], out_f)
                                           and torch.equal(staged[2], out_cluster)),
             "torch_faces_equal": bool(tf.shape == out_f.shape and torch.equal(tf, out_f)), "torch_cluster_equal": bool(torch.equal(tc, out_cluster)),
             "torch_positions_max_abs_difference": float((tv.double() - out_v.double()).abs().max()) if same_shape else None,
             "workspace_bytes": {"index": nv * 40 + nc * 16, "input_corner_list": (nv + 1) * 4 + nf * 12 if quadric else 0, "cluster": nv * 4,
                                 "representatives_and_took": nc * 13, "triples_valid_keep": nf * 14, "sort_keys_and_permutations": nf * 40,
                                 "triples_corner_list": (nc + 1) * 4 + nf * 12}}
    print(json.dumps({k: v for k, v in entry.items() if k != "all_rounds"}), flush=True)
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1184x1600", help="HxW of the sphere's depth maps")
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--voxels", default="2,4", help="cell edges in mesh voxels")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_simplify_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_simplify: needs a GPU")
    dev = torch.device("cuda:0")
    from cer_mvs_amd import mesh as ME

    H, W = (int(v) for v in args.size.lower().split("x"))
    res = args.resolution
    depths, masks, Ks, Es = sphere_scene(H, W, dev)
    voxel = 2.4 / res
    grid = ME.Grid((-1.2 + 0.013 * voxel,) * 3, voxel, (res + 1,) * 3)
    ver, fac = ME.mesh_from_depth_maps(depths, masks, Ks, Es, grid, trunc=3.0 * voxel)
    del depths, masks
    torch.cuda.empty_cache()
    result = {"rounds": args.rounds, "device": torch.cuda.get_device_name(0), "height": H, "width": W, "views": len(SPHERE_DIRS),
              "grid": {"origin": list(grid.origin), "voxel": grid.voxel, "dims": list(grid.dims)}, "cases": []}
    for k in (float(s) for s in args.voxels.split(",")):
        for representative in ("quadric", "mean"):
            result["cases"].append({"voxels": k, **measure(ver, fac, k * voxel, representative, args)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
