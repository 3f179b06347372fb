#!/usr/bin/env python
"""Durations of k_compose and of the trace by launch index mod 4, over the last `steps` launches of a rocprofv3 kernel trace (GPU box): with
event_stride 4 one class of the four is the timed frames, whose kernels leave their stamps.

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/kbench.py --child balls --steps 200
  python tools/timed_launches.py DIR 200
"""
import csv, glob, json, sys
rows = []
for f in glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True):
    rows += list(csv.DictReader(open(f)))
rows.sort(key=lambda x: int(x["Start_Timestamp"]))
steps = int(sys.argv[2])
for name in ("k_compose", "k_primary"):
    v = [(int(x["Start_Timestamp"]), int(x["End_Timestamp"])) for x in rows if name in x["Kernel_Name"]]
    t = v[-steps:]
    base = len(v) - len(t)
    cls = {}
    for i, (s, e) in enumerate(t):
        cls.setdefault((base + i) % 4, []).append((e - s) / 1e3)
    for k in sorted(cls):
        d = sorted(cls[k])
        print(json.dumps({"kernel": name, "launch_index_mod4": k, "n": len(d), "mean_us": round(sum(d) / len(d), 2), "median_us": round(d[len(d)//2], 2), "min_us": round(d[0], 2), "max_us": round(d[-1], 2)}))
