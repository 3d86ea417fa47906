"""Per-vertex mesh attributes on the 513^3 sphere case of tools/bench_mesh.py: ten analytic views of a unit sphere at 1600x1184,
the mesh of `mesh_from_depth_maps` on a cubic grid of --resolution + 1 nodes per axis (2.58 M vertices at 512), every view painted with the
linear colour 0.5 + 0.25 * p of the surface point a pixel sees.

    python tools/bench_mesh_attr.py [--size 1184x1600] [--resolution 512] [--rounds 3] [--out profiles/mesh_attr_bench.json]

Between HIP events, medians of --rounds rounds after a warm-up: the colour kernel and the normals kernel through the C ABI, the stable
`torch.sort` of the corners with its `searchsorted` (`vertex_faces`), and `vertex_colors` / `vertex_normals` as whole calls on the host clock.
Beside them the plumbing baselines: the colour contract restated in torch on the device (fp64, the contract's associations, --chunk vertices
at a time), interleaved with the kernel round by round, its bytes compared with the kernel's; and a host numpy pass for the normals (face
normals scattered with `np.add.at`, another summation order: the largest difference to the kernel is reported).  Needs a GPU."""
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


def painted(depths, masks, Ks, Es):
    """colors float32 [N,3,h,w] on the device: 0.5 + 0.25 * the surface point of every masked pixel, 0 elsewhere"""
    N, h, w = depths.shape
    dev = depths.device
    v, u = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float64), torch.arange(w, device=dev, dtype=torch.float64), indexing="ij")
    pix = torch.stack([u, v, torch.ones_like(u)], -1)
    out = torch.zeros(N, 3, h, w, device=dev, dtype=torch.float32)
    for i in range(N):
        K, E = Ks[i].to(dev, torch.float64), Es[i].to(dev, torch.float64)
        cam = (pix @ torch.linalg.inv(K).T) * depths[i].double()[..., None]
        world = (cam - E[:3, 3]) @ E[:3, :3]
        out[i] = torch.where(masks[i][None] != 0, (0.5 + 0.25 * world).permute(2, 0, 1), torch.zeros((), device=dev, dtype=torch.float64)).float()
    return out


def torch_colors(vertices, depths, masks, colors, Ks, Es, tol, views, chunk):
    """the colour contract in torch ops on the device, fp64, --chunk vertices at a time"""
    dev = vertices.device
    N, h, w = depths.shape
    K, E = Ks.to(dev, torch.float64), Es.to(dev, torch.float64)
    nv = vertices.shape[0]
    rgb = torch.empty(nv, 3, device=dev, dtype=torch.uint8)
    seen = torch.empty(nv, device=dev, dtype=torch.int32)
    for s in range(0, nv, chunk):
        p = vertices[s:s + chunk].double()
        px, py, pz = p[:, 0], p[:, 1], p[:, 2]
        total = torch.zeros(p.shape[0], 3, device=dev, dtype=torch.float64)
        count = torch.zeros(p.shape[0], device=dev, dtype=torch.int32)
        for v in views:
            e, k = E[v], K[v]
            cx = ((e[0, 0] * px + e[0, 1] * py) + e[0, 2] * pz) + e[0, 3]
            cy = ((e[1, 0] * px + e[1, 1] * py) + e[1, 2] * pz) + e[1, 3]
            cz = ((e[2, 0] * px + e[2, 1] * py) + e[2, 2] * pz) + e[2, 3]
            ux = (k[0, 0] * cx + k[0, 1] * cy) + k[0, 2] * cz
            uy = (k[1, 0] * cx + k[1, 1] * cy) + k[1, 2] * cz
            uz = (k[2, 0] * cx + k[2, 1] * cy) + k[2, 2] * cz
            x, y = ux / uz, uy / uz
            a, b = x + 0.5, y + 0.5
            ok = (uz > 0) & (a >= 0) & (a < w) & (b >= 0) & (b < h)
            zero = torch.zeros_like(a)
            xi, yi = torch.where(ok, a.floor(), zero).long(), torch.where(ok, b.floor(), zero).long()
            ok &= masks[v][yi, xi] != 0
            d = depths[v][yi, xi].double()
            ok &= torch.isfinite(d) & (d > 0)
            ok &= (d - uz).abs() <= tol
            xs, ys = torch.where(ok, x, zero), torch.where(ok, y, zero)
            x0, y0 = xs.floor(), ys.floor()
            fx, fy = xs - x0, ys - y0
            xa, xb = x0.long().clamp(0, w - 1), (x0.long() + 1).clamp(0, w - 1)
            ya, yb = y0.long().clamp(0, h - 1), (y0.long() + 1).clamp(0, h - 1)
            for ch in range(3):
                plane = colors[v, ch]
                top = (1.0 - fx) * plane[ya, xa].double() + fx * plane[ya, xb].double()
                bot = (1.0 - fx) * plane[yb, xa].double() + fx * plane[yb, xb].double()
                val = (1.0 - fy) * top + fy * bot
                total[:, ch] = torch.where(ok, total[:, ch] + val, total[:, ch])
            count += ok.int()
        q = (total / count.double()[:, None]) * 255.0
        byte = torch.where(q >= 255.0, torch.full_like(q, 255.0), torch.where(q > 0.0, q.floor(), torch.zeros_like(q)))
        rgb[s:s + chunk] = torch.where((count > 0)[:, None], byte, torch.zeros_like(byte)).to(torch.uint8)
        seen[s:s + chunk] = count
    return rgb, seen


def host_normals(v, f):
    """the normals in one host numpy pass: face normals scattered onto their three vertices, then normalised (fp64)"""
    p = v.astype(np.float64)
    n = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    s = np.zeros_like(p)
    for c in range(3):
        np.add.at(s, f[:, c], n)
    length = np.linalg.norm(s, axis=1)
    ok = (length > 0) & np.isfinite(length)
    return np.where(ok[:, None], s / np.where(ok, length, 1.0)[:, None], 0.0).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1184x1600", help="HxW of the depth maps")
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1 << 20, help="vertices per chunk of the torch restatement")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_attr_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_attr: needs a GPU")
    dev = torch.device("cuda:0")
    from cer_mvs_amd import _lib as L
    from cer_mvs_amd import mesh as ME

    H, W = (int(v) for v in args.size.lower().split("x"))
    res = args.resolution
    depths, masks, Ks, Es = sphere_scene(H, W, dev)
    colors = painted(depths, masks, Ks, Es)
    voxel = 2.4 / res
    grid = ME.Grid((-1.2 + 0.013 * voxel,) * 3, voxel, (res + 1,) * 3)
    trunc = 3.0 * voxel
    refs = list(range(len(SPHERE_DIRS)))
    ver, fac = ME.mesh_from_depth_maps(depths, masks, Ks, Es, grid, trunc=trunc)
    torch.cuda.empty_cache()
    nv, nf = int(ver.shape[0]), int(fac.shape[0])
    print(f"mesh: {nv} vertices, {nf} faces", flush=True)

    lib = L.load()
    cams = ME.forward_cams(Ks, Es).to(dev)
    vlist = torch.tensor(refs, dtype=torch.int32, device=dev)
    rgb = torch.zeros(nv, 3, device=dev, dtype=torch.uint8)
    seen = torch.zeros(nv, device=dev, dtype=torch.int32)
    nrm = torch.zeros(nv, 3, device=dev, dtype=torch.float32)
    starts, order = ME.vertex_faces(fac, nv)
    p = lambda t, dt=torch.float32: L.dev_ptr(t, "t", dt)
    st = L.cur_stream()

    def color_kernel():
        L.check(lib.cer_mesh_vertex_colors_u8(p(ver), nv, p(depths), p(masks, torch.uint8), p(colors), p(cams, torch.float64), len(refs), H, W,
                                              p(vlist, torch.int32), len(refs), trunc, p(rgb, torch.uint8), p(seen, torch.int32), st), "colors")

    def normals_kernel():
        L.check(lib.cer_mesh_vertex_normals_f32(p(ver), nv, p(fac, torch.int32), nf, p(starts, torch.int32), p(order, torch.int32), p(nrm), st), "normals")
    sort = lambda: ME.vertex_faces(fac, nv)
    base = lambda: torch_colors(ver, depths, masks, colors, Ks, Es, trunc, refs, args.chunk)
    color_kernel(), normals_kernel(), sort(), base()
    torch.cuda.synchronize()
    keys = ("color_kernel_ms", "torch_colors_ms", "corner_sort_ms", "normals_kernel_ms", "vertex_colors_call_ms", "vertex_normals_call_ms", "host_normals_ms")
    rows = {k: [] for k in keys}
    hv, hf = ver.cpu().numpy(), fac.cpu().numpy()
    for _ in range(args.rounds):
        for key, fn in (("color_kernel_ms", color_kernel), ("torch_colors_ms", base), ("corner_sort_ms", sort), ("normals_kernel_ms", normals_kernel)):
            out, ms = timed(fn)
            rows[key].append(ms)
            if key == "torch_colors_ms":
                brgb, bseen = out
        for key, fn in (("vertex_colors_call_ms", lambda: ME.vertex_colors(ver, depths, masks, colors, Ks, Es, trunc, views=refs)),
                        ("vertex_normals_call_ms", lambda: ME.vertex_normals(ver, fac))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            rows[key].append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        hn = host_normals(hv, hf)
        rows["host_normals_ms"].append(1e3 * (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in rows.items()}
    result = {"height": H, "width": W, "views": len(refs), "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
              "grid": {"origin": list(grid.origin), "voxel": grid.voxel, "dims": list(grid.dims)}, "tol": trunc, "nv": nv, "nf": nf,
              "seen_share": float((seen > 0).float().mean()), "most_views_of_a_vertex": int(seen.max()), **med, "all_rounds": rows,
              "torch_over_kernel": med["torch_colors_ms"] / med["color_kernel_ms"],
              "vertex_views_per_s": nv * len(refs) / (med["color_kernel_ms"] * 1e-3),
              "torch_rgb_bytes_equal": bool(torch.equal(brgb, rgb)), "torch_seen_equal": bool(torch.equal(bseen, seen)),
              "host_normals_max_abs_difference": float(np.abs(hn.astype(np.float64) - nrm.cpu().numpy().astype(np.float64)).max())}
    print(json.dumps({k: v for k, v in result.items() if k != "all_rounds"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
