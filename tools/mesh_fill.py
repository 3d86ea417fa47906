"""Hole filling for a mesh PLY: reads a file of `mesh.write_mesh_ply`'s form, closes every boundary loop of at most
--max-edges edges on the device (`mesh.fill_holes`: any indexed triangle mesh, not only one this project extracted) and writes the result:
the input's vertices and faces first, unchanged, then the centres and the fans.  Colours the file carries are carried through (a centre
gets its loop's integer mean); normals are recomputed on the result (`mesh.vertex_normals`) when the input had them.  A small floating
piece has a rim like any hole: remove those first (`tools/mesh_clean.py`).

    python tools/mesh_fill.py IN.ply OUT.ply --max-edges N

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
    ap.add_argument("--max-edges", type=int, required=True, help="the longest loop to close, in edges (>= 3)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_fill: needs a GPU")
    from cer_mvs_amd import mesh as ME
    v, f, normals, colors = ME.read_mesh_ply(args.src, attributes=True)
    dev = torch.device("cuda:0")
    info = {}
    ov, of, _, oc = ME.fill_holes(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), args.max_edges,
                                  colors=None if colors is None else torch.from_numpy(colors).to(dev), info=info)
    on = ME.vertex_normals(ov, of) if normals is not None else None
    ME.write_mesh_ply(args.dst, ov, of, normals=on, colors=oc)
    print(json.dumps({"out": args.dst, "vertices": int(ov.shape[0]), "faces": int(of.shape[0]), "max_edges": args.max_edges, **info,
                      "normals": on is not None, "colors": oc is not None}))


if __name__ == "__main__":
    main()
