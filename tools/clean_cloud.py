"""One point cloud through an outlier filter on the device (cer-mvs_amd/cloud_eval.py), one JSON line.

    python tools/clean_cloud.py IN.ply OUT.ply --method statistical [--k 20] [--std-ratio 2.0] [--max-dist D] [--cell C]
    python tools/clean_cloud.py IN.ply OUT.ply --method radius --radius R --min-neighbours N [--cell C]

Binary little-endian PLY files (what `reconstruct_scan` / `fusion` write): `read_ply`, the filter, `fusion.write_ply` with the kept points
in their order and their colours (white when IN.ply has none).  statistical: `remove_statistical_outliers` - a point stays iff it has k
neighbours within --max-dist (itself included; default 1 % of the bounding-box diagonal) and their mean distance is below the cloud's mean
plus --std-ratio standard deviations.  radius: `remove_radius_outliers` - a point stays iff more than --min-neighbours points lie within
--radius of it (itself included).  Needs a GPU."""
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
    ap.add_argument("--method", choices=("statistical", "radius"), required=True)
    ap.add_argument("--k", type=int, default=20, help="statistical: neighbours per point, the point included (1 .. 32)")
    ap.add_argument("--std-ratio", type=float, default=2.0, help="statistical: standard deviations above the mean that are still kept")
    ap.add_argument("--max-dist", type=float, default=None, help="statistical: the neighbours' cut-off (default: 1 %% of the bounding-box diagonal)")
    ap.add_argument("--radius", type=float, default=None, help="radius: the neighbourhood")
    ap.add_argument("--min-neighbours", type=int, default=None, help="radius: a point needs more than this many points within the radius")
    ap.add_argument("--cell", type=float, default=None, help="the grid's edge (default: a quarter of the cut-off)")
    args = ap.parse_args()
    if args.method == "radius" and (args.radius is None or args.min_neighbours is None):
        ap.error("--method radius needs --radius and --min-neighbours")
    import numpy as np
    import torch
    from cer_mvs_amd import cloud_eval as CE
    from cer_mvs_amd import fusion
    if not torch.cuda.is_available():
        raise SystemExit("clean_cloud: needs a GPU")
    xyz, rgb = CE.read_ply(args.src)
    if args.method == "statistical":
        clean = {"method": "statistical", "k": args.k, "std_ratio": args.std_ratio, "max_dist": args.max_dist}
    else:
        clean = {"method": "radius", "radius": args.radius, "min_neighbours": args.min_neighbours}
    if args.cell is not None:
        clean["cell"] = args.cell
    keep, info = CE.clean_cloud(torch.from_numpy(xyz).cuda(), clean)
    keep = keep.cpu().numpy()
    fusion.write_ply(args.dst, xyz[keep], np.full((len(keep), 3), 255, np.uint8) if rgb is None else rgb[keep])
    print(json.dumps({"in": args.src, "out": args.dst, "n_in": int(len(xyz)), **info}))


if __name__ == "__main__":
    main()
