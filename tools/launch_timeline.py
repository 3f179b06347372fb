#!/usr/bin/env python
"""Kernel durations against the launch period (GPU box): runs tools/kbench.py --child <scene> under
rocprofv3 --kernel-trace and prints, per kernel name, the launches, the mean duration and the mean distance between the
starts of consecutive launches — what a frame costs beyond the time its kernel is executing — and overlap_share: over the
timed loop (the last `steps` launches of the kernel), the share of the time in which consecutive launches of it run at once
(pipelined frames; NRAYS_PIPELINE and NRAYS_PIPELINE_DEPTH are taken from the environment), beside share_ge2 / share_ge3: the
share of that loop in which at least two / at least three launches of the kernel are running (a sweep over their starts and ends).

  python tools/launch_timeline.py balls [width height [steps]]
"""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def running_shares(t):
    """Shares of [first start, last end] of the launches `t` = [(start, end), ...] with at least 2 and at least 3 of them running."""
    ev = sorted([(s, 1) for s, _ in t] + [(e, -1) for _, e in t])  # (an end sorts before a start at the same tick)
    n, last, ge2, ge3 = 0, ev[0][0], 0, 0
    for x, d in ev:
        if n >= 2:
            ge2 += x - last
        if n >= 3:
            ge3 += x - last
        n, last = n + d, x
    span = max(1, max(e for _, e in t) - min(s for s, _ in t))
    return ge2 / span, ge3 / span


def main():
    scene = sys.argv[1] if len(sys.argv) > 1 else "balls"
    w, h = (sys.argv[2], sys.argv[3]) if len(sys.argv) > 3 else ("1920", "1080")
    steps = sys.argv[4] if len(sys.argv) > 4 else "50"
    d = tempfile.mkdtemp(prefix="nrays_tl_", dir="/tmp")
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "t", "--", sys.executable, os.path.join(ROOT, "tools", "kbench.py"),
           "--child", scene, "--steps", steps, "--width", w, "--height", h]
    r = subprocess.run(cmd, env=dict(os.environ, TMPDIR="/tmp"), cwd="/tmp", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    rows = []
    for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    if not rows:
        print(r.stdout[-2000:]); raise SystemExit(1)
    rows.sort(key=lambda x: int(x["Start_Timestamp"]))
    by = {}
    for x in rows:
        by.setdefault(x["Kernel_Name"][:60], []).append((int(x["Start_Timestamp"]), int(x["End_Timestamp"])))
    for k, v in by.items():
        dur = [e - s for s, e in v]
        per = [v[i + 1][0] - v[i][0] for i in range(len(v) - 1)]
        per = sorted(per)[: max(1, len(per) * 3 // 4)]  # drop the gaps between the timing loops
        gaps = sorted(v[i + 1][0] - v[i][1] for i in range(len(v) - 1))[: max(1, (len(v) - 1) * 3 // 4)]
        t = v[-min(len(v), int(steps)):]
        both = sum(max(0, min(t[i][1], t[i + 1][1]) - t[i + 1][0]) for i in range(len(t) - 1))
        print(json.dumps({"kernel": k, "launches": len(v), "duration_us": round(sum(dur) / len(dur) / 1e3, 2),
                          "period_us": round(sum(per) / max(len(per), 1) / 1e3, 2), "gap_us": round(sum(gaps) / max(len(gaps), 1) / 1e3, 2),
                          "timed_loop_duration_us": round(sum(e - s for s, e in t) / len(t) / 1e3, 2),
                          "overlap_share": round(both / max(1, t[-1][1] - t[0][0]), 3),
                          "share_ge2": round(running_shares(t)[0], 3), "share_ge3": round(running_shares(t)[1], 3)}))


if __name__ == "__main__":
    main()
