#!/usr/bin/env python3
"""Which library calls does a forward make, in which order, with which arguments - and what does it return?  (needs a GPU)

    python tools/forward_launches.py --out FILE [--tree ROOT] [--only a,c,...]

The proof instrument of a host-side refactor: run it on two trees (``--tree``: the repository root whose ``cer-mvs_amd`` package is
imported; default: the tree this file lies in) against the SAME library file (``CER_MVS_LIB``) and compare the two FILEs byte for byte.

Per configuration the model is built from ``synthetic.fill_state_dict`` weights and a seeded synthetic scene (the seeds of the named
golden fixture), one untraced forward packs the weights, then every input runs once the way bench.py's instrumented pass runs it:
``update.USE_PLANS = False`` inside ``_lib.timing(records)``.  Recorded per call: the entry point, every integer and float argument,
and of every pointer argument only whether it is null (ConvInputs / CopySegments: the same per field).  Recorded per forward: the
SHA-256 of the result's bytes.  Two freshly built models then repeat the inputs, one with launch plans off and one with them on.
The one with plans on must return the recorded bytes - unless the one with plans off does not either: such a configuration is not
reproducible from run to run to begin with, its digest is recorded as "not reproducible" and only its launch list is compared.
(Seen with the torch convolutions of the "LR" encoder and of forward_train before this tool asked for MIOpen's deterministic solvers,
``torch.backends.cudnn.deterministic``; with them every configuration reproduces.)

Configurations: a default model, e2e_tiny, gru_precision="s16f8"; b the same with "auto": three calibration inputs and one decided
forward (no untraced forward: it would be the first calibration input); c e2e_cfg1; d dim_fmap=128 (plain encode, tiled head, fp32
walk); e encoder_backend="miopen"; f encoder_type="LR" on e2e_lr; g aggregation=("mean", "max"), the literal path; h forward_cached
on a three-image store, equal to the ordinary forward of the same stack (recorded as well); i slab.sharded_forward on
slab.LocalExchange(2) at e2e_cfg1's size; j overflow_policy="raise"; k forward_train, train_backend "torch" and "hip" (digest over the
concatenated predictions); l ``encoder_hip.ENGINE = "tiled"`` around a default forward and around ``HipEncoder.forward_nchw`` of fnet
and cnet (digest over the three results); m gru_precision="f16x3"; n gru_precision="fp32" (l - n on e2e_tiny)."""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import numpy as np


def encode_arg(a):
    if a is None:
        return "null"
    if isinstance(a, (bool, int, float)):
        return a
    if isinstance(a, ctypes.c_void_p):
        return "ptr" if a.value else "null"
    if isinstance(a, ctypes._SimpleCData):
        return a.value
    if isinstance(a, ctypes.Array):
        return [encode_arg(x) for x in a]
    if isinstance(a, ctypes.Structure):
        n = getattr(a, "nsrc", None)
        fields = {}
        for name, ftype in a._fields_:
            v = getattr(a, name)
            if isinstance(v, ctypes.Array):
                v = list(v)[:n] if n is not None else list(v)
                v = [("ptr" if x else "null") for x in v] if issubclass(ftype._type_, ctypes.c_void_p) else [encode_arg(x) for x in v]
            fields[name] = encode_arg(v) if not isinstance(v, list) else v
        return fields
    if hasattr(a, "_obj"):                                 # ctypes.byref(x)
        return encode_arg(a._obj)
    if hasattr(a, "contents"):                             # ctypes.pointer(x)
        return encode_arg(a.contents) if a else "null"
    raise TypeError(f"forward_launches: argument of type {type(a).__name__}")


def digest(out):
    import torch
    outs = out if isinstance(out, (list, tuple)) else [out]
    return hashlib.sha256(b"".join(np.ascontiguousarray(o.detach().float().cpu().numpy()).tobytes() for o in outs)).hexdigest()


def configurations(golden_dir, only):
    """name -> (build, inputs, warm): ``build()`` returns run(input) -> tensor(s); ``inputs``: what the forwards are run on"""
    import torch
    from cer_mvs_amd import RAFT, encoder_hip, ops, slab
    from cer_mvs_amd.synthetic import fill_state_dict, synthetic_scene
    from cer_mvs_amd.update import UpdateBlock
    dev = torch.device("cuda", 0)
    scenes = {}

    def fixture(name):
        g = np.load(os.path.join(golden_dir, name + ".npz"))
        return g, [tuple(int(x) for x in c) for c in g["cascade"]]

    def scene(g, seed=None, V=None):
        key = (int(g["H"]), int(g["W"]), int(g["V"]) if V is None else V, int(g["scene_seed"]) if seed is None else seed)
        if key not in scenes:
            images, poses, intr, scale = synthetic_scene(*key[:3], seed=key[3])
            scenes[key] = (images.to(dev), poses.to(dev), intr.to(dev), scale)
        return scenes[key]

    def model(g, cascade, aggregation=None, policy=None, **kw):
        m = RAFT(cascade=cascade, **{"test_mode": True, **kw})
        if aggregation is not None:
            m.update_block = UpdateBlock(cascade=m.cascade, dim_net=64, dim_inp=64, aggregation=aggregation)
        m.load_state_dict(fill_state_dict(m.state_dict(), seed=int(g["weight_seed"])))
        if policy is not None:
            m.overflow_policy = policy
        return m.to(dev).eval()

    def plain(name, **kw):
        g, cascade = fixture(name)

        def build():
            m = model(g, cascade, **kw)
            return lambda s: m(*s[:3], scale=s[3])
        return build, g

    def cached():
        g, cascade = fixture("e2e_tiny")

        def build():
            m = model(g, cascade, gru_precision="s16f8")

            def run(s):
                h, w = s[0].shape[-2] // 4, s[0].shape[-1] // 4
                store = torch.zeros(s[0].shape[1], (h + 4) * (w + 4), 128, device=dev, dtype=torch.float16)
                m._get_engines(dev)[1].features_split(s[0][0].float(), None, store, n_ref=0, border=2, scale=0.125, raw=True,
                                                      flag=ops.overflow_flag(dev))
                f1s = ops.feat_ref_rows(store[0], h, w, border=2)
                slots = torch.arange(1, store.shape[0], device=dev, dtype=torch.int32)
                out = m.forward_cached(s[0][0, :1], f1s, store, slots, s[1], s[2], s[3]).clone()
                assert torch.equal(out, m(*s[:3], scale=s[3])), "forward_cached differs from the ordinary forward of the same stack"
                return out
            return run
        return build, g

    def sharded():
        g, cascade = fixture("e2e_cfg1")

        def build():
            m = model(g, cascade, gru_precision="s16f8")
            ex = slab.LocalExchange(2)
            return lambda s: slab.sharded_forward(m, s[0], s[1], s[2], s[3], ex)
        return build, g

    def tiled():
        g, cascade = fixture("e2e_tiny")

        def build():
            m = model(g, cascade, gru_precision="s16f8")

            def run(s):
                prev, encoder_hip.ENGINE = encoder_hip.ENGINE, "tiled"
                try:
                    x = s[0][0].float() * (2 / 255.0) - 1
                    return [m(*s[:3], scale=s[3])] + [encoder_hip.HipEncoder(net, dev).forward_nchw(x) for net in (m.fnet, m.cnet)]
                finally:
                    encoder_hip.ENGINE = prev
            return run
        return build, g

    def train(backend):
        g, cascade = fixture("train_tiny")

        def build():
            m = model(g, cascade, test_mode=False, train_backend=backend)
            return lambda s: m(*s[:3], scale=s[3])
        return build, g

    table = {
        "a": (*plain("e2e_tiny", gru_precision="s16f8"), None, True),
        "b": (*plain("e2e_tiny", gru_precision="auto"), [None, 17, 18, None], False),
        "c": (*plain("e2e_cfg1", gru_precision="s16f8"), None, True),
        "d": (*plain("e2e_tiny", gru_precision="s16f8", dim_fmap=128), None, True),
        "e": (*plain("e2e_tiny", gru_precision="s16f8", encoder_backend="miopen"), None, True),
        "f": (*plain("e2e_lr", gru_precision="s16f8", encoder_type="LR"), None, True),
        "g": (*plain("e2e_tiny", gru_precision="s16f8", aggregation=("mean", "max")), None, True),
        "h": (*cached(), None, True),
        "i": (*sharded(), None, True),
        "j": (*plain("e2e_tiny", gru_precision="s16f8", policy="raise"), None, True),
        "k_torch": (*train("torch"), None, True),
        "k_hip": (*train("hip"), None, True),
        "l": (*tiled(), None, True),
        "m": (*plain("e2e_tiny", gru_precision="f16x3"), None, True),
        "n": (*plain("e2e_tiny", gru_precision="fp32"), None, True),
    }
    for name, (build, g, seeds, warm) in table.items():
        if only and name.split("_")[0] not in only:
            continue
        V = 2 if name == "h" else None                      # (h: a store of three images)
        yield name, build, [scene(g, seed, V) for seed in (seeds or [None])], warm


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--only", default="", help="comma-separated configuration letters")
    args = ap.parse_args()
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    torch.backends.cudnn.deterministic = True              # (MIOpen's deterministic solvers for the torch convolutions of e, f, g and k)
    from cer_mvs_amd import _lib as L, update
    assert os.path.abspath(L.__file__).startswith(os.path.abspath(args.tree) + os.sep), L.__file__
    lib_sha = hashlib.sha256(open(L.LIB_PATH, "rb").read()).hexdigest()
    result = {"library_sha256": lib_sha, "configurations": {}}
    for name, build, inputs, warm in configurations(os.path.join(here, "tests", "golden"), set(filter(None, args.only.split(",")))):
        run = build()
        with torch.no_grad():
            if warm:
                run(inputs[0])
            forwards = []
            update.USE_PLANS = False
            try:
                for s in inputs:
                    recs = []
                    with L.timing(recs):
                        out = run(s)
                    forwards.append({"sha256": digest(out), "calls": [[r[0]] + [encode_arg(a) for a in r[1]] for r in recs]})
            finally:
                update.USE_PLANS = True
            again = {}
            for plans in (False, True):                    # fresh models: the same bytes with launch plans off and on
                update.USE_PLANS = plans
                try:
                    run = build()
                    if warm:
                        run(inputs[0])
                    again[plans] = [digest(run(s)) for s in inputs]
                finally:
                    update.USE_PLANS = True
            for i, f in enumerate(forwards):
                if again[False][i] != f["sha256"]:
                    f["sha256"] = "not reproducible"
                else:
                    assert again[True][i] == f["sha256"], f"configuration {name}: launch plans on gives {again[True][i]}, off {f['sha256']}"
        torch.cuda.synchronize()
        result["configurations"][name] = forwards
        print(f"{name:8s} " + "  ".join(f"{len(f['calls'])} calls {f['sha256'][:16]}" for f in forwards), flush=True)
    with open(args.out, "w") as f:                         # one call per line: the file diffs well
        f.write('{"library_sha256": "%s", "configurations": {\n' % lib_sha)
        for i, (name, forwards) in enumerate(result["configurations"].items()):
            f.write('"%s": [\n' % name)
            for j, fw in enumerate(forwards):
                f.write('{"sha256": "%s", "calls": [\n' % fw["sha256"])
                f.write(",\n".join(json.dumps(c, separators=(",", ":")) for c in fw["calls"]))
                f.write("\n]}" + (",\n" if j + 1 < len(forwards) else "\n"))
            f.write("]" + (",\n" if i + 1 < len(result["configurations"]) else "\n"))
        f.write("}}\n")
    json.load(open(args.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
