"""A point cloud from the surface of a mesh PLY: reads a file of `mesh.write_mesh_ply`'s form, draws points with a density
proportional to area on the device (`mesh.sample_mesh`: any indexed triangle mesh, not only one this project extracted) and writes them
with `fusion.write_ply`.  Exactly one of --n (that many samples), --density (samples per unit area) and --spacing (`mesh.sample_mesh_even`:
evenly spaced, pairwise farther apart than that) fixes the count.  Colours the file carries are mixed per sample from the face's corners
(black without them); --normals adds the face's unit normal of every sample.

    python tools/mesh_sample.py IN.ply OUT.ply (--n N | --density D | --spacing S) [--seed K] [--normals]

Needs a GPU."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("src")
    ap.add_argument("dst")
    how = ap.add_mutually_exclusive_group(required=True)
    how.add_argument("--n", type=int, help="the number of samples")
    how.add_argument("--density", type=float, help="samples per unit area")
    how.add_argument("--spacing", type=float, help="evenly spaced samples, pairwise farther apart than this")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--normals", action="store_true", help="write the face's unit normal of every sample")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_sample: needs a GPU")
    from cer_mvs_amd import fusion as FU
    from cer_mvs_amd import mesh as ME
    v, f, _, colors = ME.read_mesh_ply(args.src, attributes=True)
    dev = torch.device("cuda:0")
    vd, fd = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    cd = None if colors is None else torch.from_numpy(colors).to(dev)
    info = {}
    if args.spacing is not None:
        points, _, normals, cols = ME.sample_mesh_even(vd, fd, args.spacing, seed=args.seed, normals=args.normals, colors=cd, info=info)
    else:
        points, _, normals, cols, _ = ME.sample_mesh(vd, fd, n=args.n, density=args.density, seed=args.seed, normals=args.normals, colors=cd,
                                                     info=info)
    xyz = points.cpu().numpy()
    FU.write_ply(args.dst, xyz, np.zeros((len(xyz), 3), np.uint8) if cols is None else cols.cpu().numpy(),
                 normals=None if normals is None else normals.cpu().numpy())
    print(json.dumps({"out": args.dst, "vertices": int(len(v)), "faces": int(len(f)), "samples": int(len(xyz)), "seed": args.seed, **info,
                      "normals": normals is not None, "colors": cols is not None}))


if __name__ == "__main__":
    main()
