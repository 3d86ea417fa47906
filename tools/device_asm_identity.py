#!/usr/bin/env python3
"""Does the compiler emit the same gfx950 device assembly for two source trees?  (no GPU needed)

    python tools/device_asm_identity.py TREE_A TREE_B [--jobs N] [--only SUBSTR] [--kernels]

For either tree the compile commands are the ones its own csrc/Makefile prints (make -n -B) for libcermvs.so and the
variant libraries named in TARGETS, so every object gets its exact flags, target-specific additions included.  Each
`hipcc ... -c X.hip -o Y.o` is rerun as `... -fuse-cuid=none --offload-device-only -S X.hip` (without -fuse-cuid=none the
__hip_cuid_* symbol differs between any two compiles), and the two assembly texts are compared after dropping .file and
.ident lines.  One line per object: name, kernels in A, kernels in B, the two SHA-256 digests (first 16 digits) and
`same` or `DIFFERENT`; an object that only one tree builds is `ONLY-A` / `ONLY-B`.  Exit status 1 unless all are `same`.
--kernels: under an object that differs, one line per kernel symbol - `same` or `DIFFERENT` (its text from the entry label to its
.size line), then for A and B the instruction lines, .amdhsa_next_free_vgpr, .amdhsa_next_free_sgpr, the group-segment (LDS) and
the private-segment (scratch) bytes.  Counted lines and descriptor values only; which instructions they are is not looked at.
"""
import argparse
import concurrent.futures
import hashlib
import os
import re
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


KERNEL_FIELDS = (("vgpr", ".amdhsa_next_free_vgpr"), ("sgpr", ".amdhsa_next_free_sgpr"), ("lds", ".amdhsa_group_segment_fixed_size"),
                 ("scratch", ".amdhsa_private_segment_fixed_size"))


def split_kernels(lines):
    """{kernel symbol: (its lines from the entry label to its .size line, instruction lines, {field: .amdhsa_ value})} of one assembly text"""
    names = [ln.split()[1] for ln in lines if ln.lstrip().startswith(".amdhsa_kernel ")]
    out = {}
    for name in names:
        first = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        last = next(i for i in range(first, len(lines)) if lines[i].lstrip().startswith(f".size\t{name},"))
        body = lines[first:last + 1]
        code = body[1:next(i for i, ln in enumerate(body) if ln.lstrip().startswith(".section"))]
        insts = sum(1 for ln in code if ln.strip() and not ln.lstrip().startswith((".", ";")) and not ln.split(";")[0].rstrip().endswith(":"))
        vals = {}
        for ln in body:
            word = ln.split()
            for key, directive in KERNEL_FIELDS:
                if word and word[0] == directive:
                    vals[key] = word[1]
        out[name] = (body, insts, vals)
    return out


def short_name(symbol):
    """the function name of an Itanium-mangled symbol (_Z<length><name>...), or the symbol itself"""
    m = re.match(r"_Z(\d+)", symbol)
    return symbol[m.end():m.end() + int(m.group(1))] if m else symbol


def print_kernels(la, lb):
    """one line per kernel of an object that differs: same / DIFFERENT and both sides' instruction lines, registers, LDS and scratch bytes"""
    ka, kb = split_kernels(la), split_kernels(lb)
    shorts = [short_name(s) for s in dict.fromkeys(list(ka) + list(kb))]
    for sym in dict.fromkeys(list(ka) + list(kb)):
        label = short_name(sym) if shorts.count(short_name(sym)) == 1 else sym
        if sym not in ka or sym not in kb:
            print(f"    {label:40s} {'ONLY-A' if sym in ka else 'ONLY-B'}")
            continue
        (ba, ia, va), (bb, ib, vb) = ka[sym], kb[sym]
        fields = "  ".join(f"{key} {va.get(key, '?')} {vb.get(key, '?')}" for key, _ in KERNEL_FIELDS)
        print(f"    {label:40s} {'same     ' if ba == bb else 'DIFFERENT'}  insts {ia} {ib}  {fields}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--only", default="", help="objects whose name contains this")
    ap.add_argument("--keep", default=None, help="directory that receives A_<object>.s / B_<object>.s of differing objects")
    ap.add_argument("--kernels", action="store_true", help="under a differing object, one line per kernel")
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
            if not same and args.kernels:
                print_kernels(la, lb)
            if not same and args.keep:
                os.makedirs(args.keep, exist_ok=True)
                for side, lines in (("A", la), ("B", lb)):
                    with open(os.path.join(args.keep, f"{side}_{o.replace('/', '_')}.s"), "w") as f:
                        f.write("\n".join(lines) + "\n")
    print(f"{len(objs) - bad} of {len(objs)} objects same")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
