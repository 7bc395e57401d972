"""Mean of one rocprofv3 counter per dispatch, by kernel name.

usage: pmc_by_kernel.py DIR OUT.json [COUNTER]      (DIR: the -d directory of a `rocprofv3 --pmc COUNTER --kernel-trace` run)

tools/pmc_traffic.py tells a step's launches apart by position and therefore profiles single steps; this one groups by name, so it
also works on runs of steps replayed as graphs -- where the two instances of the small nets' wgrad+adam launch (k_small_tn_desc,
k_small_tn_nograd) both appear.  WRITE_SIZE / FETCH_SIZE come in KiB and are reported in bytes."""
import csv
import glob
import json
import sys

d, out = sys.argv[1], sys.argv[2]
counter = sys.argv[3] if len(sys.argv) > 3 else "WRITE_SIZE"
f = glob.glob(d + "/**/*counter_collection.csv", recursive=True)[0]
acc = {}
for r in csv.DictReader(open(f)):
    if r["Counter_Name"] != counter:
        continue
    a = acc.setdefault(r["Kernel_Name"].split("(")[0], [0, 0.0])
    a[0] += 1
    a[1] += float(r["Counter_Value"])
scale = 1024 if counter.endswith("_SIZE") else 1
res = {n: {"dispatches": c, ("bytes_mean" if scale > 1 else "mean"): round(v / c * scale, 1)} for n, (c, v) in sorted(acc.items())}
with open(out, "w") as fo:
    json.dump({"counter": counter, "kernels": res}, fo, indent=1)
for n, v in res.items():
    print(n, v)
