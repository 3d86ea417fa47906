"""Vertex normals for a mesh PLY: reads a file of `mesh.write_mesh_ply`'s form, computes area-weighted vertex normals on the
device (`mesh.vertex_normals`: any indexed triangle mesh, not only one this project extracted) and writes the mesh back with nx ny nz; colours
the file carries are kept.

    python tools/mesh_normals.py IN.ply OUT.ply

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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_normals: needs a GPU")
    from cer_mvs_amd import mesh as ME
    v, f, _, colors = ME.read_mesh_ply(args.src, attributes=True)
    dev = torch.device("cuda:0")
    normals = ME.vertex_normals(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)).cpu().numpy()
    ME.write_mesh_ply(args.dst, v, f, normals=normals, colors=colors)
    print(json.dumps({"out": args.dst, "vertices": len(v), "faces": len(f), "without_normal": int((~normals.any(1)).sum()),
                      "colors": colors is not None}))


if __name__ == "__main__":
    main()
