"""Two point clouds, one JSON line: DTU's accuracy / completeness / overall and Tanks-and-Temples' precision / recall / F-score of A (the
prediction) against B (the ground truth), on the device (cer-mvs_amd/cloud_eval.py).

    python tools/compare_clouds.py A.ply B.ply [--max-dist 20.0] [--tau 2.0] [--thin 0.2] [--thin-method voxel|greedy] [--thin-seed 0]
                                   [--align none|icp|icp-plane] [--align-max-dist D] [--align-voxel V [V ...]] [--align-normals-k K] [--init T.txt]

Binary little-endian PLY files (what `reconstruct_scan` / `fusion` write).  --thin: thin A first - --thin-method voxel (the default): one point
per cell of that edge; greedy: the DTU script's own reduction, `radius_thin` with that radius, visiting the points in the random order of
--thin-seed.  --align icp: A is first registered onto B with point-to-point ICP (`register`) - one stage per
--align-voxel edge on the voxel-thinned clouds, coarse to fine, then one on the clouds as they are, every stage matching within
--align-max-dist (default --max-dist), from the 4x4 of --init (a text file `numpy.loadtxt` reads; default the identity) - and moved by the
result before anything is measured; the JSON line gains "T", "align_iterations" (all stages), "align_converged", "align_fitness" and "align_rmse" (the last
stage's).  --align icp-plane: the same stages with point-to-plane ICP (`register(method="plane")`) on B's normals, estimated once
on the whole of B from --align-normals-k neighbours (default 20); the line then also carries "align_method": "plane" and "align_rmse_point", and
"align_rmse" is the plane residual's.  With --align none (the default) --init alone moves A.  Crop volumes, observability masks and ground planes of the benchmarks are the
caller's business.  Needs a GPU."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a", help="predicted cloud (PLY)")
    ap.add_argument("b", help="ground-truth cloud (PLY)")
    ap.add_argument("--max-dist", type=float, default=20.0, help="distances at or beyond this leave the means (DTU: 20 mm)")
    ap.add_argument("--tau", type=float, default=None, help="F-score threshold (default: max_dist / 10)")
    ap.add_argument("--thin", type=float, default=None, help="voxel edge / radius for thinning A")
    ap.add_argument("--thin-method", choices=("voxel", "greedy"), default="voxel", help="voxel_downsample or radius_thin (the DTU script's)")
    ap.add_argument("--thin-seed", type=int, default=0, help="seed of the greedy thinning's visiting order")
    ap.add_argument("--align", choices=("none", "icp", "icp-plane"), default="none", help="register A onto B first (point-to-point / point-to-plane ICP)")
    ap.add_argument("--align-max-dist", type=float, default=None, help="matching distance of the registration (default: --max-dist)")
    ap.add_argument("--align-voxel", type=float, nargs="+", default=[], help="voxel edges of the coarse stages, coarse to fine")
    ap.add_argument("--align-normals-k", type=int, default=20, help="neighbours behind B's normals (--align icp-plane)")
    ap.add_argument("--init", default=None, help="text file with the 4x4 initial motion of A (numpy.loadtxt)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from cer_mvs_amd import cloud_eval as CE
    if not torch.cuda.is_available():
        raise SystemExit("compare_clouds: needs a GPU")
    tau = args.max_dist / 10 if args.tau is None else args.tau
    a = torch.from_numpy(CE.read_ply(args.a)[0]).cuda()
    b = torch.from_numpy(CE.read_ply(args.b)[0]).cuda()
    out = {"a": args.a, "b": args.b, "max_dist": args.max_dist, "thin": args.thin, "thin_method": args.thin_method, "thin_seed": args.thin_seed}
    T = None if args.init is None else np.loadtxt(args.init, dtype=np.float64)
    if args.align != "none":
        reach = args.max_dist if args.align_max_dist is None else args.align_max_dist
        plane = {"method": "plane", "normals": {"k": args.align_normals_k}} if args.align == "icp-plane" else {}
        reg = CE.register(a, b, [(v, reach, 50) for v in args.align_voxel] + [(None, reach, 50)], init=T, **plane)
        T = reg["T"]
        out.update(T=T.tolist(), align_iterations=sum(st["iterations"] for st in reg["stages"]), align_converged=reg["converged"],
                   align_fitness=reg["fitness"], align_rmse=reg["rmse"])
        if plane:
            out.update(align_method="plane", align_rmse_point=reg["rmse_point"])
    if T is not None:
        a = CE.rigid_transform(a, T)
    out.update(CE.accuracy_completeness(a, b, max_dist=args.max_dist, thin=args.thin, thin_method=args.thin_method, thin_seed=args.thin_seed))
    if args.thin is not None:                                # (the same selection again, for the F-score)
        a = a.index_select(0, CE.radius_thin(a, args.thin, seed=args.thin_seed) if args.thin_method == "greedy" else CE.voxel_downsample(a, args.thin))
    out.update({k: v for k, v in CE.fscore(a, b, tau).items() if k in ("precision", "recall", "fscore", "tau")})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
