"""The exact distance of every point of a cloud to the surface of a mesh, on the device (`mesh.mesh_distances`).

    python tools/mesh_distance.py MESH.ply CLOUD.ply OUT.npy [--max-dist 20.0] [--cell C]

MESH.ply: a file of `mesh.write_mesh_ply`'s form; CLOUD.ply: a binary little-endian cloud.  OUT.npy: float32 [n], the distance of every point
to the nearest triangle within --max-dist, inf where there is none.  --cell: the edge of the index's cells (default: from the mesh's mean
face area and --max-dist; the distances do not depend on it).  Prints one JSON line: the files, "max_dist", "n", "within" (points with a
face within --max-dist), "mean" (of those) and the index's "cell", "pairs", "faces_indexed" and "cells".  Needs a GPU."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mesh", help="the mesh (PLY)")
    ap.add_argument("cloud", help="the points to measure (PLY)")
    ap.add_argument("out", help="the distances (npy, float32 [n])")
    ap.add_argument("--max-dist", type=float, default=20.0, help="faces farther than this are not looked for (inf in the output)")
    ap.add_argument("--cell", type=float, default=None, help="edge of the index's cells")
    args = ap.parse_args()
    import numpy as np
    import torch
    from cer_mvs_amd import cloud_eval as CE
    from cer_mvs_amd import mesh as ME
    if not torch.cuda.is_available():
        raise SystemExit("mesh_distance: needs a GPU")
    v, f = ME.read_mesh_ply(args.mesh)
    points = torch.from_numpy(CE.read_ply(args.cloud)[0]).cuda()
    info = {}
    dist = ME.mesh_distances(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), points, args.max_dist, cell=args.cell, info=info).cpu().numpy()
    np.save(args.out, dist)
    near = dist[np.isfinite(dist)].astype(np.float64)
    print(json.dumps(dict(mesh=args.mesh, cloud=args.cloud, out=args.out, max_dist=args.max_dist, n=int(len(dist)), within=int(len(near)),
                          mean=float(near.mean()) if len(near) else None, **info)))


if __name__ == "__main__":
    main()
