"""Per kernel of a rocprofv3 kernel trace (the *_kernel_trace.csv of `rocprofv3 --kernel-trace -f csv`):
launches, median / min / max duration in us, total and share, by total time.  Every launch of the
traced process counts, a warm-up's included.

  python3 tools/trace_medians.py TRACE.csv
"""
import csv
import re
import statistics
import sys
from collections import defaultdict

d = defaultdict(list)
with open(sys.argv[1]) as f:
    for row in csv.DictReader(f):
        d[row["Kernel_Name"]].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
tot = sum(sum(v) for v in d.values())
print(f"{'kernel':70s} {'calls':>6s} {'median us':>10s} {'min':>8s} {'max':>8s} {'total ms':>9s} {'share':>6s}")
for k, v in sorted(d.items(), key=lambda kv: -sum(kv[1])):
    m = re.search(r"([A-Za-z0-9_]+_kernel)(<[^(]*>)?", k)
    name = (m.group(1) + (m.group(2) or "") if m else k)[:70]
    print(f"{name:70s} {len(v):6d} {statistics.median(v):10.2f} {min(v):8.2f} {max(v):8.2f} {sum(v) / 1e3:9.3f} {100 * sum(v) / tot:5.1f}%")
