"""Vertex-clustering simplification for a mesh PLY: reads a file of `mesh.write_mesh_ply`'s form, merges the vertices inside
every cell of edge --cell on the device (`mesh.simplify_vertex_clustering`: any indexed triangle mesh, not only one this project extracted)
into the cell's quadric minimiser or mean, drops the faces that collapse and the duplicates, and writes the rest back.  Colours the file
carries are carried through (the members' mean); normals are recomputed on the result (`mesh.vertex_normals`) when the input had them or
--normals is given.

    python tools/mesh_simplify.py IN.ply OUT.ply --cell C [--representative mean|quadric] [--normals]

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
    ap.add_argument("--cell", type=float, required=True, help="edge of a clustering cell, in the mesh's units")
    ap.add_argument("--representative", choices=("quadric", "mean"), default="quadric")
    ap.add_argument("--normals", action="store_true", help="write vertex normals even if the input had none")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_simplify: needs a GPU")
    from cer_mvs_amd import mesh as ME
    v, f, normals, colors = ME.read_mesh_ply(args.src, attributes=True)
    dev = torch.device("cuda:0")
    put = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    info = {}
    sv, sf, _, sc = ME.simplify_vertex_clustering(put(v), put(f), args.cell, representative=args.representative, colors=put(colors), info=info)
    sn = ME.vertex_normals(sv, sf) if (normals is not None or args.normals) else None
    ME.write_mesh_ply(args.dst, sv, sf, normals=sn, colors=sc)
    print(json.dumps({"out": args.dst, "vertices": int(sv.shape[0]), "faces": int(sf.shape[0]), "read": [len(v), len(f)], "cell": args.cell,
                      "representative": args.representative, **info, "normals": sn is not None, "colors": colors is not None}))


if __name__ == "__main__":
    main()
