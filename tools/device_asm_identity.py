#!/usr/bin/env python3
"""Does the compiler emit the same gfx950 device assembly for two source trees?  (no GPU needed)

    python tools/device_asm_identity.py TREE_A TREE_B [--jobs N] [--only SUBSTR]

For either tree the compile commands are the ones its own csrc/Makefile prints (make -n -B) for libcermvs.so and the
variant libraries named in TARGETS, so every object gets its exact flags, target-specific additions included.  Each
`hipcc ... -c X.hip -o Y.o` is rerun as `... -fuse-cuid=none --offload-device-only -S X.hip` (without -fuse-cuid=none the
__hip_cuid_* symbol differs between any two compiles), and the two assembly texts are compared after dropping .file and
.ident lines.  One line per object: name, kernels in A, kernels in B, the two SHA-256 digests (first 16 digits) and
`same` or `DIFFERENT`; an object that only one tree builds is `ONLY-A` / `ONLY-B`.  Exit status 1 unless all are `same`.
"""
import argparse
import concurrent.futures
import hashlib
import os
import shlex
import subprocess
import sys

TARGETS = ["libcermvs.so", "variants/libcermvs_optin.so", "variants/libcermvs_sxtrace.so", "variants/libcermvs_fuzz.so"]


def compile_commands(tree):
    """{object name: argv that writes the object's device assembly to stdout}, in the tree's csrc directory"""
    csrc = os.path.join(tree, "cer-mvs_amd", "csrc")
    out = subprocess.run(["make", "-n", "-B"] + TARGETS, cwd=csrc, check=True, capture_output=True, text=True).stdout
    cmds = {}
    for line in out.splitlines():
        argv = shlex.split(line)
        if "-c" not in argv or not argv[argv.index("-c") + 1].endswith(".hip"):
            continue                                       # links, mkdir, the host-only pack.cpp
        obj = argv[argv.index("-o") + 1]
        del argv[argv.index("-o"):argv.index("-o") + 2]
        argv[argv.index("-c")] = "-S"
        cmds.setdefault(obj, argv + ["-fuse-cuid=none", "--offload-device-only", "-o", "-"])
    return csrc, cmds


def device_asm(csrc, argv):
    run = subprocess.run(argv, cwd=csrc, capture_output=True, text=True)
    if run.returncode:
        sys.exit(f"{csrc}: {' '.join(argv)}\n{run.stderr}")
    text = run.stdout
    lines = [ln for ln in text.splitlines() if not ln.lstrip().startswith((".file", ".ident"))]
    kernels = sum(1 for ln in lines if ln.lstrip().startswith(".amdhsa_kernel "))
    return kernels, hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16], lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--only", default="", help="objects whose name contains this")
    ap.add_argument("--keep", default=None, help="directory that receives A_<object>.s / B_<object>.s of differing objects")
    args = ap.parse_args()
    (dir_a, cmd_a), (dir_b, cmd_b) = compile_commands(args.tree_a), compile_commands(args.tree_b)
    objs = [o for o in dict.fromkeys(list(cmd_a) + list(cmd_b)) if args.only in o]
    with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
        fut = {(side, o): pool.submit(device_asm, d, c[o])
               for side, d, c in (("A", dir_a, cmd_a), ("B", dir_b, cmd_b)) for o in objs if o in c}
        bad = 0
        for o in objs:
            if (("A", o) in fut) != (("B", o) in fut):
                print(f"{o:34s} {'ONLY-A' if ('A', o) in fut else 'ONLY-B'}")
                bad += 1
                continue
            (ka, da, la), (kb, db, lb) = fut[("A", o)].result(), fut[("B", o)].result()
            same = la == lb
            bad += not same
            print(f"{o:34s} kernels {ka:3d} {kb:3d}  {da} {db}  {'same' if same else 'DIFFERENT'}", flush=True)
            if not same and args.keep:
                os.makedirs(args.keep, exist_ok=True)
                for side, lines in (("A", la), ("B", lb)):
                    with open(os.path.join(args.keep, f"{side}_{o.replace('/', '_')}.s"), "w") as f:
                        f.write("\n".join(lines) + "\n")
    print(f"{len(objs) - bad} of {len(objs)} objects same")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
