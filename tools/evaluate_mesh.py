"""A mesh against a ground-truth cloud, one JSON line: DTU's accuracy / completeness / overall and Tanks-and-Temples' precision / recall /
F-score of evenly spaced samples of the mesh's surface against the cloud, on the device (`mesh.evaluate_mesh`).

    python tools/evaluate_mesh.py MESH.ply GT.ply --spacing S [--max-dist 20.0] [--tau T] [--seed 0] [--align none|icp|icp-plane]
                                  [--method samples|exact]

MESH.ply: a file of `mesh.write_mesh_ply`'s form; GT.ply: a binary little-endian cloud.  --spacing: the samples are pairwise farther apart
than this (`mesh.sample_mesh_even`); the figures on the ground truth's side (completeness, recall) are distances to samples, not to the
surface, and carry an upward bias of up to about the spacing - take it well below --tau, or take --method exact: the ground truth's side
is then the exact distance of every cloud point to the mesh's triangles (`mesh.MeshIndex`) and the line gains "method".  --tau: the F-score's threshold (default
--max-dist / 10).  --align icp / icp-plane: the samples are first registered onto the cloud (`cloud_eval.register`, one stage on the clouds
as they are, matching within --max-dist; icp-plane on the cloud's normals from 20 neighbours) and the mesh is measured after that motion;
the line gains "T", "align_iterations", "align_converged", "align_fitness" and "align_rmse".  Needs a GPU."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mesh", help="the mesh (PLY)")
    ap.add_argument("gt", help="ground-truth cloud (PLY)")
    ap.add_argument("--spacing", type=float, required=True, help="spacing of the surface samples")
    ap.add_argument("--max-dist", type=float, default=20.0, help="distances at or beyond this leave the means (DTU: 20 mm)")
    ap.add_argument("--tau", type=float, default=None, help="F-score threshold (default: max_dist / 10)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the samples")
    ap.add_argument("--align", choices=("none", "icp", "icp-plane"), default="none", help="register the samples onto GT first")
    ap.add_argument("--method", choices=("samples", "exact"), default="samples", help="the ground truth's side: against samples, or the exact distance to the triangles")
    args = ap.parse_args()
    import torch
    from cer_mvs_amd import cloud_eval as CE
    from cer_mvs_amd import mesh as ME
    if not torch.cuda.is_available():
        raise SystemExit("evaluate_mesh: needs a GPU")
    tau = args.max_dist / 10 if args.tau is None else args.tau
    v, f = ME.read_mesh_ply(args.mesh)
    vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    gt = torch.from_numpy(CE.read_ply(args.gt)[0]).cuda()
    out = {"mesh": args.mesh, "gt": args.gt, "max_dist": args.max_dist, "seed": args.seed}
    T = None
    if args.align != "none":
        samples = ME.sample_mesh_even(vd, fd, args.spacing, seed=args.seed)[0]
        plane = {"method": "plane", "normals": {"k": 20}} if args.align == "icp-plane" else {}
        reg = CE.register(samples, gt, [(None, args.max_dist, 50)], **plane)
        T = reg["T"]
        out.update(T=T.tolist(), align_iterations=sum(st["iterations"] for st in reg["stages"]), align_converged=reg["converged"],
                   align_fitness=reg["fitness"], align_rmse=reg["rmse"])
    out.update(ME.evaluate_mesh(vd, fd, gt, args.spacing, max_dist=args.max_dist, tau=tau, seed=args.seed, align=T, method=args.method))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
