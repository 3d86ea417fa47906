"""Taubin or Laplacian smoothing for a mesh PLY: reads a file of `mesh.write_mesh_ply`'s form, smooths its vertices on the
device (`mesh.smooth_mesh`: any indexed triangle mesh, not only one this project extracted) and writes it back with the faces untouched.
Colours the file carries are carried through; normals are recomputed on the result (`mesh.vertex_normals`) when the input had them or
--normals is given.

    python tools/mesh_smooth.py IN.ply OUT.ply --iterations N [--method taubin|laplacian] [--lam L] [--mu M] [--boundary fixed|free] [--normals]

Needs a GPU."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--iterations", type=int, required=True)
    ap.add_argument("--method", choices=("taubin", "laplacian"), default="taubin")
    ap.add_argument("--lam", type=float, default=0.5, help="the weight of the shrinking step, in (0, 1]")
    ap.add_argument("--mu", type=float, default=-0.53, help="the weight of Taubin's inflating step, below -lam")
    ap.add_argument("--boundary", choices=("fixed", "free"), default="fixed", help="whether the vertices on a boundary edge stay where they are")
    ap.add_argument("--normals", action="store_true", help="write vertex normals even if the input had none")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_smooth: needs a GPU")
    from cer_mvs_amd import mesh as ME
    v, f, normals, colors = ME.read_mesh_ply(args.src, attributes=True)
    dev = torch.device("cuda:0")
    info = {}
    fd = torch.from_numpy(f).to(dev)
    sv = ME.smooth_mesh(torch.from_numpy(v).to(dev), fd, args.iterations, method=args.method, lam=args.lam, mu=args.mu, boundary=args.boundary, info=info)
    sn = ME.vertex_normals(sv, fd) if (normals is not None or args.normals) else None
    ME.write_mesh_ply(args.dst, sv, f, normals=sn, colors=colors)
    print(json.dumps({"out": args.dst, "vertices": len(v), "faces": len(f), "iterations": args.iterations, "method": args.method, "lam": args.lam,
                      "mu": args.mu, "boundary": args.boundary, **info, "normals": sn is not None, "colors": colors is not None}))


if __name__ == "__main__":
    main()
