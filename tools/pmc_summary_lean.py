"""Condense rocprofv3 --pmc passes over the lean FASTQ scan: python tools/pmc_summary_lean.py <dir> <tag> reads
<dir>/<tag>_pmc_*/**/pmc_counter_collection.csv and writes <dir>/<tag>_pmc_sq_k_fused_lean.csv (average per dispatch)."""
import collections, csv, glob, sys

d, tag = sys.argv[1], sys.argv[2]
acc = collections.defaultdict(list)
for f in glob.glob(f"{d}/{tag}_pmc_*/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if "k_fused<exg::FastqFormat, 0>" in r["Kernel_Name"]:
            acc[r["Counter_Name"]].append(float(r["Counter_Value"]))
with open(f"{d}/{tag}_pmc_sq_k_fused_lean.csv", "w") as out:
    out.write("counter,average_per_dispatch,dispatches\n")
    for k, v in sorted(acc.items()):
        print(k, sum(v) / len(v), len(v))
        out.write(f"{k},{sum(v) / len(v)},{len(v)}\n")
