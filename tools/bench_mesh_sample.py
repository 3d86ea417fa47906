"""Mesh surface sampling on the 513^3 sphere case of tools/bench_mesh.py: ten analytic views of a unit sphere at 1600x1184, the
mesh of `mesh_from_depth_maps` on a cubic grid of --resolution + 1 nodes per axis (2.58 M vertices and 5.15 M faces at 512).

    python tools/bench_mesh_sample.py [--size 1184x1600] [--resolution 512] [--rounds 3] [--n 1000000,10000000] [--host-n 1000000]
                                      [--out profiles/mesh_sample_bench.json]

Medians of --rounds interleaved rounds after a warm-up, between HIP events unless said otherwise: the table (areas, weights, `cumsum` and the
two host reads), the sample kernel alone at every n (points and faces only, and with normals, colours and uv), the same contract in torch
ops on the device - `torch.searchsorted` on the prefix sums with the same targets, the gathers of the corners and the fp64 combination, which
must give the same points - a host numpy pass of the whole contract (Philox included) at --host-n on the host clock, `sample_mesh` as a whole
call and `sample_mesh_even` at a spacing of two voxels on the host clock.  The kernel's rate is stated in samples and in dependent search
steps per second: the search is ceil(log2(nf)) dependent reads of a table of 8 nf bytes, not a stream.  Needs a GPU."""
import argparse
import json
import math
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

M32 = np.uint64(0xffffffff)
S32 = np.uint64(32)


def philox_words(seed, offset, n):
    """Philox4x32-10 of the counters (k, 0, 0) under the key ``seed``, numpy uint64 -> four uint64 arrays of 32-bit words"""
    k = np.arange(n, dtype=np.uint64) + np.uint64(offset)
    c = [k & M32, k >> S32, np.zeros(n, np.uint64), np.zeros(n, np.uint64)]
    k0, k1 = seed & 0xffffffff, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & M32, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    return c


def mulhi64(r, W):
    """floor(r * W / 2^64) for uint64 r and an integer W < 2^63, by 32-bit halves"""
    rh, rl, wh, wl = r >> S32, r & M32, np.uint64(W >> 32), np.uint64(W & 0xffffffff)
    mid = (rl * wl >> S32) + (rh * wl & M32) + (rl * wh & M32)
    return rh * wh + (rh * wl >> S32) + (rl * wh >> S32) + (mid >> S32)


def host_pass(ver64, fac, cum, W, seed, n):
    """the whole contract in numpy on the host -> (points float32 [n,3], face)"""
    x0, x1, x2, x3 = philox_words(seed, 0, n)
    t = mulhi64((x0 << S32) | x1, W).astype(np.int64)
    face = np.searchsorted(cum, t, side="right")
    a, b = x2.astype(np.int64), x3.astype(np.int64)
    fold = a + b >= 1 << 32
    a, b = np.where(fold, 0xffffffff - a, a), np.where(fold, 0xffffffff - b, b)
    u, v = ((a.astype(np.float64) + 0.5) * 2.0 ** -32)[:, None], ((b.astype(np.float64) + 0.5) * 2.0 ** -32)[:, None]
    w = (1.0 - u) - v
    f = fac[face]
    return ((w * ver64[f[:, 0]] + u * ver64[f[:, 1]]) + v * ver64[f[:, 2]]).astype(np.float32), face.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1184x1600", help="HxW of the sphere's depth maps")
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--n", default="1000000,10000000")
    ap.add_argument("--host-n", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_sample_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_sample: needs a GPU")
    dev = torch.device("cuda:0")
    from cer_mvs_amd import mesh as ME

    H, Wd = (int(v) for v in args.size.lower().split("x"))
    res = args.resolution
    counts = [int(v) for v in args.n.split(",")]
    depths, masks, Ks, Es = sphere_scene(H, Wd, dev)
    voxel = 2.4 / res
    grid = ME.Grid((-1.2 + 0.013 * voxel,) * 3, voxel, (res + 1,) * 3)
    ver, fac = ME.mesh_from_depth_maps(depths, masks, Ks, Es, grid, trunc=3.0 * voxel)
    del depths, masks
    torch.cuda.empty_cache()
    nv, nf = int(ver.shape[0]), int(fac.shape[0])
    col = torch.randint(0, 256, (nv, 3), device=dev, dtype=torch.uint8, generator=torch.Generator(dev).manual_seed(1))
    cum, W, shift, with_weight = ME._sample_table(ver, fac, nv, nf)
    area = math.ldexp(float(W), -shift)
    steps = math.ceil(math.log2(nf))
    print(f"{nv} vertices, {nf} faces; area {area:.6f} (4 pi = {4 * math.pi:.6f}), shift {shift}, {with_weight} faces with weight, {steps} search steps, "
          f"table {8 * nf / 1e6:.1f} MB", flush=True)
    ver64 = ver.double()
    fac64 = fac.long()
    held = {}

    def kernel(n, full):
        return ME._draw(ver, fac, nv, nf, cum, 0, 0, None, n, full, col if full else None, full)

    def prepare(n):
        """the targets and barycentrics of the n samples, on the device: the inputs of the torch form"""
        x0, x1, _, _ = philox_words(0, 0, n)
        t = torch.from_numpy(mulhi64((x0 << S32) | x1, W).astype(np.int64)).to(dev)
        p, face, _, _, uv = ME._draw(ver, fac, nv, nf, cum, 0, 0, None, n, False, None, True)
        held[n] = (t, uv[:, 0:1].contiguous(), uv[:, 1:2].contiguous(), p, face)

    def torch_form(n):
        t, u, v, _, _ = held[n]
        face = torch.searchsorted(cum, t, right=True)
        f = fac64.index_select(0, face)
        w = (1.0 - u) - v
        p = ((w * ver64.index_select(0, f[:, 0]) + u * ver64.index_select(0, f[:, 1])) + v * ver64.index_select(0, f[:, 2])).float()
        return p, face

    spacing = 2.0 * voxel

    def whole(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, 1e3 * (time.perf_counter() - t0)

    for n in counts:                                         # warm-up, and the inputs of the torch form
        prepare(n)
        kernel(n, True)
        torch_form(n)
    ME._sample_table(ver, fac, nv, nf)
    ME.sample_mesh(ver, fac, n=counts[0])
    ME.sample_mesh_even(ver, fac, spacing)
    torch.cuda.synchronize()
    rows = {}
    for _ in range(args.rounds):                             # interleaved: every path in every round
        rows.setdefault("table_ms", []).append(timed(lambda: ME._sample_table(ver, fac, nv, nf))[1])
        rows.setdefault("face_areas_ms", []).append(timed(lambda: ME._areas(ver, fac, nv, nf))[1])
        for n in counts:
            rows.setdefault(f"kernel_{n}_ms", []).append(timed(lambda: kernel(n, False))[1])
            rows.setdefault(f"kernel_full_{n}_ms", []).append(timed(lambda: kernel(n, True))[1])
            rows.setdefault(f"torch_{n}_ms", []).append(timed(lambda: torch_form(n))[1])
            rows.setdefault(f"sample_mesh_call_{n}_ms", []).append(whole(lambda: ME.sample_mesh(ver, fac, n=n))[1])
        rows.setdefault("sample_mesh_even_call_ms", []).append(whole(lambda: ME.sample_mesh_even(ver, fac, spacing))[1])
    med = {k: statistics.median(v) for k, v in rows.items()}
    same = {}
    for n in counts:
        t, _, _, p, face = held[n]
        tp, tface = torch_form(n)
        same[str(n)] = bool(torch.equal(tp.view(torch.int32), p.view(torch.int32)) and torch.equal(tface.int(), face))
    hv, hf, hc = ver.cpu().numpy().astype(np.float64), fac.cpu().numpy(), cum.cpu().numpy()
    host_ms = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        hp, hface = host_pass(hv, hf, hc, W, 0, args.host_n)
        host_ms.append(1e3 * (time.perf_counter() - t0))
    dp, dface, _, _, _ = ME._draw(ver, fac, nv, nf, cum, 0, 0, None, args.host_n, False, None, False)
    host_same = bool(np.array_equal(hp.view(np.uint32), dp.cpu().numpy().view(np.uint32)) and np.array_equal(hface, dface.cpu().numpy()))
    einfo = {}
    ME.sample_mesh_even(ver, fac, spacing, info=einfo)
    rates = {str(n): {"samples_per_s": n / (1e-3 * med[f"kernel_{n}_ms"]), "search_steps_per_s": n * steps / (1e-3 * med[f"kernel_{n}_ms"]),
                      "speedup_over_torch": med[f"torch_{n}_ms"] / med[f"kernel_{n}_ms"]} for n in counts}
    result = {"rounds": args.rounds, "device": torch.cuda.get_device_name(0), "height": H, "width": Wd, "views": len(SPHERE_DIRS),
              "grid": {"origin": list(grid.origin), "voxel": grid.voxel, "dims": list(grid.dims)}, "nv": nv, "nf": nf, "area": area, "shift": shift,
              "faces_with_weight": with_weight, "search_steps": steps, "table_bytes": 8 * nf, "medians_ms": med, "all_rounds_ms": rows,
              "kernel_rates": rates, "torch_form_gives_the_same_points": same, "host_n": args.host_n, "host_numpy_ms": statistics.median(host_ms),
              "host_numpy_all_ms": host_ms, "host_numpy_gives_the_same_points": host_same, "even_spacing": spacing, "even_info": einfo}
    print(json.dumps({k: v for k, v in result.items() if k != "all_rounds_ms"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
