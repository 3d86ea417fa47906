#!/usr/bin/env python3
"""What do the drivers above a forward write and return?  (needs a GPU)

    python tools/driver_outputs.py --out FILE [--tree ROOT] [--only map,inference,...]

The proof instrument of a refactor of the driver layer (pipeline.py, inference.py, scan.py, the driver half of fusion.py), in the style of
tools/forward_launches.py: run it on two trees (``--tree``: the repository root whose ``cer-mvs_amd`` package is imported; default: the
tree this file lies in) against the SAME library file (``CER_MVS_LIB``) and compare the two FILEs byte for byte.

The scan is synthetic and seeded (``synthetic.synthetic_scene``: 6 views of 128x160, four source views per reference view, a scale per
view), the weights are hashed (``synthetic.fill_state_dict``), the cascade and the pinned arithmetic form are those of
tests/test_scan_gpu.py.  Recorded per configuration: the sorted relative names of the files written with the SHA-256 of each, and
the SHA-256 of every returned array (scalars and lists as they are).

Configurations: ``map`` DepthMapPipeline.map over 7 stacks on 2 streams; ``inference`` with 1 and 3 streams, at rescale 1 and at rescale 2
with crop (64, 128), both with write_min_depth; ``inference_scan`` with the same settings, cached and force_uncached; ``auto``
inference_scan with a gru_precision="auto" model on 3 streams (also: every replica's auto_choice, read as the session closes);
``depths`` ScanSession.depths; ``fusion`` fusion.fusion on the PFMs of inference_scan; ``reconstruct`` reconstruct_scan with
write=True, write_depths=True - one pass, rescale=(1, 2), clean={"method": "statistical", "k": 8}, normals=True."""
import argparse
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

CASCADE = [(64, 64, 3), (-1, 320, 3)]
H, W, M, NF = 128, 160, 6, 4
SETTINGS = {"s1": dict(rescale=1, crop=None), "s2crop": dict(rescale=2, crop=(64, 128))}


def sha(a):
    import torch
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.ascontiguousarray(a)
    return f"{a.dtype.str}{list(a.shape)}:" + hashlib.sha256(a.tobytes()).hexdigest()


def tree_of(folder):
    """sorted relative file names under ``folder`` -> SHA-256 of the bytes"""
    out = {}
    for root, _, files in os.walk(folder):
        for f in files:
            p = os.path.join(root, f)
            out[os.path.relpath(p, folder).replace(os.sep, "/")] = hashlib.sha256(open(p, "rb").read()).hexdigest()
    return dict(sorted(out.items()))


def returned(v):
    import torch
    if isinstance(v, (np.ndarray, torch.Tensor)):
        return sha(v)
    if isinstance(v, dict):
        return {str(k): returned(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [returned(x) for x in v]
    if isinstance(v, (np.floating, np.integer, np.bool_)):
        return v.item()
    return v


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--only", default="", help="comma-separated configuration groups")
    args = ap.parse_args()
    only = set(filter(None, args.only.split(",")))
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    from cer_mvs_amd import RAFT, _lib as L, fusion, scan
    from cer_mvs_amd.inference import inference
    from cer_mvs_amd.pipeline import DepthMapPipeline
    from cer_mvs_amd.synthetic import fill_state_dict, synthetic_scene
    assert os.path.abspath(L.__file__).startswith(os.path.abspath(args.tree) + os.sep), L.__file__
    assert torch.cuda.is_available(), "driver_outputs: needs a GPU"
    dev = torch.device("cuda", 0)

    def model(pinned=True):
        kw = dict(gru_precision="s16f8", enc_precision="f16x3", cost_precision="x3") if pinned else {}
        m = RAFT(cascade=CASCADE, test_mode=True, **kw)
        m.load_state_dict(fill_state_dict(m.state_dict(), seed=9))
        return m.to(dev).eval()

    images, poses, intr, scale = synthetic_scene(H, W, M - 1, seed=4)
    images, poses, intr = images[0], poses[0], intr[0]
    names = [f"{i:08d}" for i in range(M)]
    pairs = [[(i + d) % M for d in (2, 5, 1, 3)] for i in range(M)]
    scales = [scale * (1.0 + 0.01 * i) for i in range(M)]

    def loader():
        """what the reference's loader yields, one reference view at a time, backed by the scan's arrays"""
        for i in range(M):
            idx = [i] + pairs[i]
            yield images[idx][None].clone(), poses[idx][None].clone(), intr[idx][None].clone(), [names[i]], scales[i]

    def rel(files, folder):
        return [os.path.relpath(f, folder).replace(os.sep, "/") for f in files]

    result = {}

    def record(name, value):
        result[name] = value
        print(f"{name:40s} {hashlib.sha256(json.dumps(value, sort_keys=True).encode()).hexdigest()[:16]}", flush=True)

    def want(group):
        return not only or group in only

    with tempfile.TemporaryDirectory() as tmp:
        if want("map"):
            pipe = DepthMapPipeline(model(), streams=2)
            items = []
            for n in range(7):
                idx = [n % M] + pairs[n % M]
                items.append((images[idx][None].to(dev), poses[idx][None].to(dev), intr[idx][None].to(dev), scales[n % M]))
            with torch.no_grad():
                record("map_streams2", [sha(d) for d in pipe.map(items)])
            assert pipe.check_overflow() == 0
            pipe.close()
        for key, st in SETTINGS.items():
            for streams in (1, 3):
                if want("inference"):
                    out = os.path.join(tmp, f"inference_{key}_{streams}")
                    files = inference(loader(), None, os.path.join(out, "o"), model=model(), num_frames=NF, streams=streams,
                                      write_min_depth=os.path.join(out, "min"), **st)
                    record(f"inference_{key}_streams{streams}", {"returned": rel(files, out), "files": tree_of(out)})
                for forced in (False, True):
                    if want("inference_scan"):
                        out = os.path.join(tmp, f"scan_{key}_{streams}_{forced}")
                        tm = {}
                        files = scan.inference_scan(model(), images, poses, intr, names, pairs, scales, os.path.join(out, "o"), num_frames=NF,
                                                    streams=streams, write_min_depth=os.path.join(out, "min"), force_uncached=forced, timings=tm, **st)
                        assert tm["cached"] == (not forced)
                        record(f"inference_scan_{key}_streams{streams}_{'uncached' if forced else 'cached'}",
                               {"returned": rel(files, out), "files": tree_of(out)})
        if want("auto"):
            out = os.path.join(tmp, "auto")
            choices = []
            plain_close = scan.ScanSession.close

            def close(self):                               # (close() drops the replicas: read their decisions first)
                choices.append([m.auto_choice for m in self.pipe.models])
                plain_close(self)
            scan.ScanSession.close = close
            try:
                files = scan.inference_scan(model(pinned=False), images, poses, intr, names, pairs, scales, os.path.join(out, "o"),
                                            num_frames=NF, streams=3)
            finally:
                scan.ScanSession.close = plain_close
            record("inference_scan_auto_streams3", {"returned": rel(files, out), "files": tree_of(out), "auto_choice": choices})
        if want("depths"):
            for streams in (1, 3):
                sess = scan.ScanSession(model(), images, poses, intr, streams=streams)
                try:
                    record(f"depths_streams{streams}", sha(sess.depths(pairs, scales, num_frames=NF)))
                finally:
                    sess.close()
        if want("fusion"):
            out = os.path.join(tmp, "fusion")
            scan.inference_scan(model(), images, poses, intr, names, pairs, scales, out, num_frames=NF, streams=3)
            views = []
            for i in range(M):
                idx = [i] + pairs[i]
                views.append((images[idx][None].clone(), poses[idx][None].clone(), intr[idx][None].clone(), [(names[j],) for j in idx], None))
            got = fusion.fusion(views, out, suffix=f"_scale1_nf{NF}", glb=0.25)
            record("fusion", {"returned": returned(got), "files": tree_of(out)})
        if want("reconstruct"):
            forms = {"one_pass": {}, "two_pass": {"rescale": (1, 2)}, "clean": {"clean": {"method": "statistical", "k": 8}},
                     "normals": {"normals": True}}
            for key, kw in forms.items():
                out = os.path.join(tmp, f"reconstruct_{key}")
                got = scan.reconstruct_scan(model(), images, poses, intr, names, pairs, scales, out, num_frames=NF, streams=3,
                                            write=True, write_depths=True, **kw)
                record(f"reconstruct_{key}", {"returned": returned(got), "files": tree_of(out)})
    torch.cuda.synchronize()
    lib_sha = hashlib.sha256(open(L.LIB_PATH, "rb").read()).hexdigest()
    with open(args.out, "w") as f:
        json.dump({"library_sha256": lib_sha, "configurations": result}, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
