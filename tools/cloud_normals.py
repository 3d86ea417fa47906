"""Surface normals for one point cloud on the device (cer-mvs_amd/cloud_eval.py estimate_normals), one JSON line.

    python tools/cloud_normals.py IN.ply OUT.ply [--k 20] [--max-dist D] [--cell C] [--viewpoint X Y Z]

Binary little-endian PLY files (what `reconstruct_scan` / `fusion` write): `read_ply`, `estimate_normals`, `fusion.write_ply` with the points
in their order, their colours (white when IN.ply has none) and `nx ny nz`.  The normal of a point is the direction of least spread of its
--k nearest neighbours within --max-dist (itself included; default 1 % of the bounding-box diagonal); a point without three neighbours
that span a plane gets (0, 0, 0).  --viewpoint turns every normal towards that position (a camera centre, a scanner); without it the
component of largest magnitude is positive.  Needs a GPU."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("src", metavar="IN.ply")
    ap.add_argument("dst", metavar="OUT.ply")
    ap.add_argument("--k", type=int, default=20, help="neighbours per point, the point included (1 .. 32)")
    ap.add_argument("--max-dist", type=float, default=None, help="the neighbours' cut-off (default: 1 %% of the bounding-box diagonal)")
    ap.add_argument("--cell", type=float, default=None, help="the grid's edge (default: a quarter of the cut-off)")
    ap.add_argument("--viewpoint", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="turn the normals towards this position")
    args = ap.parse_args()
    import numpy as np
    import torch
    from cer_mvs_amd import cloud_eval as CE
    from cer_mvs_amd import fusion
    if not torch.cuda.is_available():
        raise SystemExit("cloud_normals: needs a GPU")
    xyz, rgb = CE.read_ply(args.src)
    vp = None if args.viewpoint is None else torch.tensor(args.viewpoint, dtype=torch.float32, device="cuda")
    info = {}
    normal, curvature = CE.estimate_normals(torch.from_numpy(xyz).cuda(), k=args.k, max_dist=args.max_dist, cell=args.cell, viewpoints=vp, info=info)
    fusion.write_ply(args.dst, xyz, np.full((len(xyz), 3), 255, np.uint8) if rgb is None else rgb, normals=normal.cpu().numpy())
    curv = curvature[~torch.isnan(curvature)]
    print(json.dumps({"in": args.src, "out": args.dst, "n": int(len(xyz)), **info, "viewpoint": args.viewpoint,
                      "median_curvature": float(curv.median()) if len(curv) else None}))


if __name__ == "__main__":
    main()
