"""Mesh components and small-piece removal on two meshes:

  sphere  the 513^3 sphere case of tools/bench_mesh.py / bench_mesh_attr.py: ten analytic views of a unit sphere at 1600x1184, the mesh of
          `mesh_from_depth_maps` on a cubic grid of --resolution + 1 nodes per axis (2.58 M vertices at 512), ONE component, in slot order.
          The selection keeps every second face.
  noise   a seeded random volume of --noise^3 nodes (uniform values, a quarter of the nodes unobserved), extracted by `extract_mesh`: many
          small components.  The selection is `remove_small_components(min_faces=--min-faces)`'s.

    python tools/bench_mesh_clean.py [--size 1184x1600] [--resolution 512] [--noise 129] [--min-faces 64] [--rounds 3] [--out profiles/mesh_clean_bench.json]

Between HIP events, medians of --rounds rounds after a warm-up: the label sweeps through the C ABI from fresh labels (as many as
`mesh_components` needed, one call, no host read: the time per sweep), the stable `torch.sort` of the corners with its `searchsorted`
(`vertex_faces`), the selection's count call (the count launch and the scan), its emit call (vertex emit, face emit) and the gather of
normals and colours by `index`; and `mesh_components`, `select_faces` and `remove_small_components` as whole calls on the host clock.  Beside
them the baselines, interleaved round by round and compared with the kernels' results: the same contract restated in torch ops on the
device (labels to a fixed point by `scatter_reduce_(amin)` with one host read per step; the selection by a boolean scatter and a cumulative
sum), and a host pass (`scipy.sparse.csgraph.connected_components` where scipy is installed, else the union-find of
tests/mesh_clean_reference.py) that includes the copy of the faces to the host.  Needs a GPU."""
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


def torch_roots(faces, nv):
    """every vertex's root by torch ops on the device: the contract's sweep, synchronous (every step reads the previous step's labels)"""
    dev = faces.device
    labels = torch.arange(nv, device=dev, dtype=torch.int64)
    idx = faces.long()
    steps = 0
    while True:
        steps += 1
        twice = labels[labels]
        m = twice[idx].min(1).values
        new = twice.clone()
        for c in range(3):
            new.scatter_reduce_(0, idx[:, c], m, "amin")
        if torch.equal(new, labels):                         # the step's host read
            return labels, steps
        labels = new


def torch_components(faces, nv):
    labels, steps = torch_roots(faces, nv)
    roots = torch.nonzero(labels == torch.arange(nv, device=faces.device)).reshape(-1)
    return torch.searchsorted(roots, labels).to(torch.int32), steps


def torch_select(vertices, faces, keep):
    kept = faces[keep.bool()].long()
    used = torch.zeros(vertices.shape[0], device=vertices.device, dtype=torch.bool)
    used[kept.reshape(-1)] = True
    new = torch.cumsum(used, 0) - 1
    index = torch.nonzero(used).reshape(-1)
    return vertices[index], new[kept].to(torch.int32), index.to(torch.int32)


def host_components(faces, nv):
    """vertex_component on the host, numbered by ascending root, from device faces (the copy is part of the pass)"""
    f = faces.cpu().numpy()
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        rows = np.concatenate([f[:, 0], f[:, 0]])
        cols = np.concatenate([f[:, 1], f[:, 2]])
        graph = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(nv, nv)).tocsr()
        _, lab = connected_components(graph, directed=False)
        how = "scipy.sparse.csgraph.connected_components"
    except ImportError:
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import mesh_clean_reference as C
        lab = C.vertex_roots(f, nv)
        how = "union-find (tests/mesh_clean_reference.py)"
    first = np.full(int(lab.max()) + 1 if nv else 0, nv, dtype=np.int64)      # renumber by the smallest vertex of every label
    np.minimum.at(first, lab, np.arange(nv))
    return np.searchsorted(np.sort(first), first[lab]).astype(np.int32), how


def measure(name, ver, fac, keep_of, args):
    from cer_mvs_amd import _lib as L
    from cer_mvs_amd import mesh as ME
    lib, dev = L.load(), ver.device
    nv, nf = int(ver.shape[0]), int(fac.shape[0])
    info = {}
    vc, fc, n_faces, n_vertices = ME.mesh_components(fac, nv, info=info)
    sweeps = info["sweeps"]
    keep = keep_of(fc, n_faces).to(torch.uint8).contiguous()
    print(f"{name}: {nv} vertices, {nf} faces, {info['components']} components, {sweeps} sweeps", flush=True)
    nrm = ME.vertex_normals(ver, fac)
    col = (ver.abs() * 40.0).clamp(0.0, 255.0).to(torch.uint8)
    starts, order = ME.vertex_faces(fac, nv)
    p = lambda t, dt=torch.float32: L.dev_ptr(t, "t", dt)
    st = L.cur_stream()
    labels = torch.empty(nv, device=dev, dtype=torch.int32)
    flags = torch.zeros(sweeps, device=dev, dtype=torch.int32)
    fresh = torch.arange(nv, device=dev, dtype=torch.int32)

    def sweep_call():
        L.check(lib.cer_mesh_label_sweeps_i32(p(fac, torch.int32), nf, p(starts, torch.int32), p(order, torch.int32), nv, p(labels, torch.int32),
                                              p(flags, torch.int32), sweeps, st), "sweeps")
    P = int(lib.cer_mesh_select_partials(nv, nf))
    used = torch.empty(nv, device=dev, dtype=torch.uint8)
    partials = torch.empty(P, device=dev, dtype=torch.int32)
    offsets = torch.empty(P + 2, device=dev, dtype=torch.int64)
    totals = torch.zeros(2, device=dev, dtype=torch.int64)
    vmap = torch.empty(nv, device=dev, dtype=torch.int32)

    def count_call():
        L.check(lib.cer_mesh_select_count(p(fac, torch.int32), nf, p(starts, torch.int32), p(order, torch.int32), nv, p(keep, torch.uint8),
                                          p(used, torch.uint8), p(partials, torch.int32), p(offsets, torch.int64), p(totals, torch.int64), st), "count")
    count_call()
    nvo, nfo = (int(v) for v in totals.cpu())
    out_v = torch.empty(nvo, 3, device=dev)
    out_f = torch.empty(nfo, 3, device=dev, dtype=torch.int32)
    index = torch.empty(nvo, device=dev, dtype=torch.int32)

    def emit_call():
        L.check(lib.cer_mesh_select_emit_f32(p(ver), nv, p(fac, torch.int32), nf, p(keep, torch.uint8), p(used, torch.uint8), p(offsets, torch.int64),
                                             nvo, nfo, p(vmap, torch.int32), p(out_v) if nvo else None, p(index, torch.int32) if nvo else None,
                                             p(out_f, torch.int32) if nfo else None, st), "emit")

    def gather():
        g = index.long()
        return nrm.index_select(0, g), col.index_select(0, g)
    sort = lambda: ME.vertex_faces(fac, nv)
    labels.copy_(fresh), sweep_call(), emit_call(), gather(), sort(), torch_components(fac, nv), torch_select(ver, fac, keep)
    torch.cuda.synchronize()
    roots_after = labels.clone()
    keys = ("sweeps_ms", "torch_components_ms", "corner_sort_ms", "select_count_ms", "select_emit_ms", "attribute_gather_ms", "torch_select_ms",
            "mesh_components_call_ms", "select_faces_call_ms", "remove_small_components_call_ms", "host_components_ms")
    rows = {k: [] for k in keys}
    for _ in range(args.rounds):
        labels.copy_(fresh)
        flags.zero_()
        for key, fn in (("sweeps_ms", sweep_call), ("torch_components_ms", lambda: torch_components(fac, nv)), ("corner_sort_ms", sort),
                        ("select_count_ms", count_call), ("select_emit_ms", emit_call), ("attribute_gather_ms", gather),
                        ("torch_select_ms", lambda: torch_select(ver, fac, keep))):
            out, ms = timed(fn)
            rows[key].append(ms)
            if key == "torch_components_ms":
                tvc, tsteps = out
            if key == "torch_select_ms":
                tsel = out
        for key, fn in (("mesh_components_call_ms", lambda: ME.mesh_components(fac, nv)), ("select_faces_call_ms", lambda: ME.select_faces(ver, fac, keep, nrm, col)),
                        ("remove_small_components_call_ms", lambda: ME.remove_small_components(ver, fac, min_faces=args.min_faces, normals=nrm, colors=col))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            rows[key].append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        hvc, how = host_components(fac, nv)
        rows["host_components_ms"].append(1e3 * (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in rows.items()}
    flag_list = flags.cpu().tolist()
    entry = {"nv": nv, "nf": nf, "components": info["components"], "largest_components_faces": sorted(n_faces.cpu().tolist(), reverse=True)[:8],
             "sweeps": sweeps, "sweeps_that_changed_a_label": int(sum(flag_list)), "ms_per_sweep": med["sweeps_ms"] / sweeps,
             "torch_steps": tsteps, "kept_faces": nfo, "kept_vertices": nvo, **med, "all_rounds": rows,
             "torch_over_sweeps": med["torch_components_ms"] / med["sweeps_ms"], "host_pass": how,
             "sweeps_reach_the_roots": bool(torch.equal(roots_after, labels)) and bool((labels[labels.long()] == labels).all()),
             "torch_components_equal": bool(torch.equal(tvc, vc)), "host_components_equal": bool(np.array_equal(hvc, vc.cpu().numpy())),
             "torch_select_equal": bool(torch.equal(tsel[0].view(torch.int32), out_v.view(torch.int32)) and torch.equal(tsel[1], out_f) and torch.equal(tsel[2], index)),
             "workspace_bytes": {"labels": nv * 4, "corner_list": (nv + 1) * 4 + nf * 12, "used_and_vmap": nv * 5, "partials_and_offsets": P * 12 + 16}}
    print(json.dumps({k: v for k, v in entry.items() if k != "all_rounds"}), flush=True)
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1184x1600", help="HxW of the sphere's depth maps")
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--noise", type=int, default=129, help="nodes per axis of the noise volume")
    ap.add_argument("--min-faces", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_clean_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_clean: needs a GPU")
    dev = torch.device("cuda:0")
    from cer_mvs_amd import mesh as ME

    H, W = (int(v) for v in args.size.lower().split("x"))
    result = {"rounds": args.rounds, "device": torch.cuda.get_device_name(0), "min_faces": args.min_faces}

    n = args.noise
    gen = torch.Generator(device="cpu").manual_seed(7)
    tsdf = (torch.rand(n, n, n, generator=gen) * 2.0 - 1.0).to(dev)
    weight = (torch.rand(n, n, n, generator=gen) >= 0.25).to(torch.int32).to(dev)
    ver, fac = ME.extract_mesh(tsdf, weight, ME.Grid((0.0, 0.0, 0.0), 1.0, (n, n, n)))
    del tsdf, weight
    result["noise"] = {"nodes": [n, n, n], "unobserved_share": 0.25, "seed": 7,
                       **measure("noise", ver, fac, lambda fc, n_faces: n_faces[fc.long()] >= args.min_faces, args)}
    del ver, fac
    torch.cuda.empty_cache()

    res = args.resolution
    depths, masks, Ks, Es = sphere_scene(H, W, dev)
    voxel = 2.4 / res
    grid = ME.Grid((-1.2 + 0.013 * voxel,) * 3, voxel, (res + 1,) * 3)
    ver, fac = ME.mesh_from_depth_maps(depths, masks, Ks, Es, grid, trunc=3.0 * voxel)
    del depths, masks
    torch.cuda.empty_cache()
    result["sphere"] = {"height": H, "width": W, "views": len(SPHERE_DIRS), "grid": {"origin": list(grid.origin), "voxel": grid.voxel, "dims": list(grid.dims)},
                        **measure("sphere", ver, fac, lambda fc, n_faces: torch.arange(fc.shape[0], device=fc.device) % 2 == 0, args)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
