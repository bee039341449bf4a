#!/usr/bin/env python3
"""How much of the wavefront path's shading runs beside another frame's traversal: two figures from one kernel trace.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 bench.py --steps 30
    scripts/wf_overlap.py DIR [--frames 30]

(no --pmc and no other tracing domain in that run: they serialise or slow the dispatches.)  Read: every *kernel_trace.csv under DIR.
The window is the timed region of the run: from the end of the wf_gather preceding the last `--frames` ones (the barrier after the
warm-up frames; the wall time starts at the first kernel after it) to the end of the last wf_gather.  A kernel that straddles an edge of
the window counts with the part of its interval that lies inside.  An interval in the trace opens when the dispatch is taken up, not when
its first wave starts: it includes the time the kernel's blocks wait for CUs.  A frame's kernels all run on its scene's stream, so "another
frame" is another stream (the Stream_Id column; Queue_Id where the trace has no stream ids).  Printed:
  - the share of the wf_shade + wf_gather busy time during which a wf_ts of ANOTHER stream is running;
  - the share of the window's wall time in which no kernel runs at all;
and, for orientation, the busy time per kernel and frame and the wall time per frame.
"""
import argparse
import csv
import glob
import os
import sys


def union(iv):
    """Sorted disjoint union of (start, end) intervals."""
    out = []
    for s, e in sorted(iv):
        if out and s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return out


def covered(s, e, u):
    """Length of [s, e) inside the disjoint sorted union u."""
    return sum(max(0, min(e, b) - max(s, a)) for a, b in u if a < e and b > s)


def kind(name):
    n = name.replace("void ", "").split("(")[0].split("<")[0].strip()
    return n if n in ("wf_ts", "wf_shade", "wf_gather", "wf_background") else "other"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("dir")
    ap.add_argument("--frames", type=int, default=30, help="timed frames of the run (bench.py --steps)")
    a = ap.parse_args()
    rows, fields = [], set()
    for f in glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            fields |= set(r)
            rows.append(r)
    if not rows:
        raise SystemExit("no *kernel_trace.csv under %s" % a.dir)
    key = "Stream_Id" if "Stream_Id" in fields and len({r["Stream_Id"] for r in rows if kind(r["Kernel_Name"]) == "wf_ts"}) > 1 else "Queue_Id"
    ks = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind(r["Kernel_Name"]), r.get(key, "")) for r in rows)
    gathers = sorted(k[1] for k in ks if k[2] == "wf_gather")
    if len(gathers) <= a.frames:
        raise SystemExit("%d wf_gather launches in the trace: fewer than --frames + 1" % len(gathers))
    t_prev, t1 = gathers[-a.frames - 1], gathers[-1]
    win = sorted((max(k[0], t_prev), min(k[1], t1), k[2], k[3]) for k in ks if k[1] > t_prev and k[0] < t1)
    t0 = win[0][0]
    wall = t1 - t0
    streams = sorted({k[3] for k in win if k[2] == "wf_ts"})
    ts_of = {s: union([(k[0], k[1]) for k in win if k[2] == "wf_ts" and k[3] == s]) for s in streams}
    busy, beside = 0, 0
    for s, e, n, st in win:
        if n not in ("wf_shade", "wf_gather"):
            continue
        busy += e - s
        beside += covered(s, e, union([tuple(x) for o in streams if o != st for x in ts_of[o]]))
    all_busy = sum(b - x for x, b in union([(k[0], k[1]) for k in win]))
    print("trace: %d kernels in the window of the last %d frames, %.3f ms wall = %.3f ms per frame; %d streams with wf_ts launches (by %s)" % (
        len(win), a.frames, wall / 1e6, wall / 1e6 / a.frames, len(streams), key))
    for n in ("wf_ts", "wf_shade", "wf_gather", "wf_background", "other"):
        sel = [k for k in win if k[2] == n]
        if sel:
            print("  %-14s %5.1f launches and %8.1f us busy per frame" % (n, len(sel) / a.frames, sum(k[1] - k[0] for k in sel) / 1e3 / a.frames))
    print("wf_shade + wf_gather busy time beside a wf_ts of another stream: %.1f %% (%.1f of %.1f us per frame)" % (
        100.0 * beside / max(1, busy), beside / 1e3 / a.frames, busy / 1e3 / a.frames))
    print("wall time in which no kernel runs: %.1f %% (%.1f us per frame)" % (100.0 * (wall - all_busy) / max(1, wall), (wall - all_busy) / 1e3 / a.frames))
    return 0


if __name__ == "__main__":
    sys.exit(main())
