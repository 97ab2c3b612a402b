"""usage: tools/features_kernel_times.py <kernel_trace.csv> <export_timing.json> [runs of the traced run]
The kExportFeatures dispatches of a `rocprofv3 --kernel-trace` run of tools/features_timing.py (mode export), in start order, cut into the requests of the timing run's
`sequence`: per request 2 + runs dispatches (the call that makes the tensor, the warm-up, the timed calls); the first two are left out.  Per request: the kernel's
median / min / max time, the bytes it moves (from the timing run) and the rate and the fraction of the 6.29 TB/s copy rate that the median gives.  Prints JSON."""
import csv
import json
import statistics
import sys

rows = [r for r in csv.DictReader(open(sys.argv[1])) if "kExportFeatures" in r["Kernel_Name"]]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
timing = json.load(open(sys.argv[2]))
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 10
seq = timing["sequence"]
assert len(rows) == len(seq) * (runs + 2), (len(rows), len(seq), runs)
out = {}
for i, name in enumerate(seq):
    chunk = rows[i * (runs + 2):(i + 1) * (runs + 2)]
    kernels = {r["Kernel_Name"].split("kExportFeatures")[1].split("(")[0] for r in chunk}
    assert len(kernels) == 1, kernels
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in chunk[2:]]
    med, nbytes = statistics.median(us), timing[name]["bytes"]
    out[name] = dict(kernel="kExportFeatures" + kernels.pop(), dispatches=len(us), kernel_us_median=round(med, 2), kernel_us_min=round(min(us), 2), kernel_us_max=round(max(us), 2),
                     bytes=nbytes, bytes_per_s=round(nbytes / (med * 1e-6)), fraction_of_copy_rate=round(nbytes / (med * 1e-6) / 6.29e12, 4),
                     call_wall_ms_median=timing[name]["median_ms"], workgroups=int(chunk[0]["Grid_Size_X"]) // 256)
print(json.dumps(out, indent=1))
