"""Small-piece removal for a mesh PLY: reads a file of `mesh.write_mesh_ply`'s form, finds the connected components on the device
(`mesh.remove_small_components`: any indexed triangle mesh, not only one this project extracted; pieces that share a vertex index are one
component), keeps those with at least --min-faces faces that are among the --keep-largest largest, and writes the rest back; normals and
colours the file carries are carried through.

    python tools/mesh_clean.py IN.ply OUT.ply [--min-faces N] [--keep-largest K]

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
    ap.add_argument("--min-faces", type=int, default=None, help="keep components with at least this many faces")
    ap.add_argument("--keep-largest", type=int, default=None, help="keep at most this many components, the largest first")
    args = ap.parse_args()
    if args.min_faces is None and args.keep_largest is None:
        ap.error("give --min-faces or --keep-largest (or both)")
    if not torch.cuda.is_available():
        raise SystemExit("mesh_clean: needs a GPU")
    from cer_mvs_amd import mesh as ME
    v, f, normals, colors = ME.read_mesh_ply(args.src, attributes=True)
    dev = torch.device("cuda:0")
    put = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    info = {}
    cv, cf, _, cn, cc = ME.remove_small_components(put(v), put(f), min_faces=args.min_faces, keep_largest=args.keep_largest, normals=put(normals),
                                                   colors=put(colors), info=info)
    ME.write_mesh_ply(args.dst, cv, cf, normals=cn, colors=cc)
    print(json.dumps({"out": args.dst, "vertices": int(cv.shape[0]), "faces": int(cf.shape[0]), "read": [len(v), len(f)], **info,
                      "normals": normals is not None, "colors": colors is not None}))


if __name__ == "__main__":
    main()
