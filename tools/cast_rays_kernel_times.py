"""usage: tools/cast_rays_kernel_times.py <directory of a rocprofv3 --kernel-trace run (csv) around tools/cast_rays_timing.py ... cast ...> [calls per request]
Per kernel name of the ray queries -- kCastLoad, kTraceWide (by instantiation), kCastResolve -- the number of dispatches and the total, median, minimum and maximum
duration in microseconds, and each kernel's share of the three kernels' total.  With the calls per request (the timing script makes 2 + runs per entry of its
`sequence`: one that makes the tensors, one warm-up, the timed ones) also `by_request`: per entry, in dispatch order, the median of each of the three kernels.
Prints one JSON line."""
import csv
import glob
import json
import os
import re
import statistics
import sys

rows = []
for path in glob.glob(os.path.join(sys.argv[1], "**", "*kernel_trace.csv"), recursive=True):
    with open(path, newline="") as f:
        rows += list(csv.DictReader(f))
by = {}
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
order = []
for r in rows:
    name = r.get("Kernel_Name") or r.get("kernel_name") or ""
    if not re.search(r"kCast|kTraceWide", name):
        continue
    short = re.sub(r"^void ", "", name.replace("rf::(anonymous namespace)::", "")).split("(")[0]
    by.setdefault(short, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    order.append((re.match(r"k[A-Za-z]+", short).group(0), by[short][-1]))
total = sum(sum(v) for v in by.values()) or 1.0
out = {k: dict(dispatches=len(v), total_us=round(sum(v), 2), median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2),
               share=round(sum(v) / total, 4)) for k, v in sorted(by.items())}
if len(sys.argv) > 2:
    per = int(sys.argv[2])
    calls = [order[i:i + 3] for i in range(0, len(order), 3)]          # one call = kCastLoad, kTraceWide, kCastResolve
    assert all([k for k, _ in c] == ["kCastLoad", "kTraceWide", "kCastResolve"] for c in calls), "the trace is not a sequence of single-chunk calls"
    out["by_request"] = [{k: round(statistics.median(c[j][1] for c in calls[g:g + per]), 2) for j, k in enumerate(("kCastLoad", "kTraceWide", "kCastResolve"))}
                         for g in range(0, len(calls), per)]
print(json.dumps(out))
