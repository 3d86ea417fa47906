#!/bin/bash
# Issue counters of the cost volume's tile kernel (two-term form) at the bench shapes: two rocprofv3 --pmc passes over tools/prof_build.py,
# counters only (no tracing flags), averaged over the launches of both stages.  The table behind profiles/cost_lines_issue_ab.json.
# usage: tools/pmc_cost_lines.sh <tag> [library]      (A/B: run it once per library build, on the same box)
# The profiled program is started directly behind "--"; its settings travel in the environment.
tag=${1:-run}; [ -n "$2" ] && export CER_MVS_LIB=$2
export CER_COST_X2=1
out=${PMC_OUT:-/tmp/pmc_cost_lines}; mkdir -p "$out/$tag"
for set in "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS GRBM_GUI_ACTIVE" "SQ_ACTIVE_INST_ANY SQ_WAVE_CYCLES SQ_LDS_BANK_CONFLICT SQ_INSTS_VMEM_RD"; do
  d=$out/$tag/$(echo $set | tr ' ' '_')
  timeout -k 10 300 rocprofv3 --pmc $set --kernel-include-regex "cost_lines_kernel<3, false>" -f csv -d "$d" -o x -- python tools/prof_build.py > "$d.log" 2>&1 || { echo "pass failed: $d.log"; exit 1; }
  python - "$d" "$tag" <<'PY'
import collections, csv, glob, sys
agg, n = collections.defaultdict(float), collections.defaultdict(int)
for f in glob.glob(sys.argv[1] + "/**/x_counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if "cost_lines_kernel<3, false>" in r["Kernel_Name"]:
            agg[r["Counter_Name"]] += float(r["Counter_Value"]); n[r["Counter_Name"]] += 1
for k in sorted(agg):
    print(f"{sys.argv[2]} {k:28s} launches {n[k]:3d}  avg {agg[k] / n[k]:.6g}")
PY
done
