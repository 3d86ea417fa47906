"""What a mesh PLY is: reads a file of `mesh.write_mesh_ply`'s form and prints `mesh.mesh_topology`'s report as one JSON line -
vertices, faces, edges, boundary / non-manifold / inconsistently oriented edges, boundary vertices and loops, unreferenced vertices,
degenerate faces, the Euler characteristic, and whether the mesh is closed, edge-manifold and oriented.

    python tools/mesh_topology.py IN.ply

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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_topology: needs a GPU")
    from cer_mvs_amd import mesh as ME
    v, f = ME.read_mesh_ply(args.src)
    print(json.dumps(ME.mesh_topology(torch.from_numpy(f).to(torch.device("cuda:0")), len(v))))


if __name__ == "__main__":
    main()
