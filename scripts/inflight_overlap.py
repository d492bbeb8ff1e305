#!/usr/bin/env python3
"""How much the kernels of different events overlap, from a kernel trace of bench.py with several events in flight.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py --gpus 1 --steps 30 --warmup 5 --no-cpu-baseline
    python scripts/inflight_overlap.py DIR [--skip 106] [--count 35]

(a run of its own: no counters in the same run.)  bench.py launches from one host thread, event after event, so in dispatch order
everything from one k_event_init up to the next belongs to one event.  --skip / --count choose the events looked at: with bench.py's
defaults events 6 .. 140 run with the others in flight (100 set-up events, then 5 warm-up and 30 timed steps: events 106 .. 140, the
default window), the ten after them alone.

Per kernel name: launches, mean duration, the share of its duration during which a kernel of ANOTHER event runs, and the share
during which it is the only kernel on the GPU.  Then the busy time of the GPU per event: the union of all kernel intervals of the
window, divided by the events in it -- with perfect overlap of E events that is the step time, with none it is the sum of the
critical paths."""
import argparse
import csv
import glob
import os
import sys


def _col(row, *names):
    for n in names:
        if n in row:
            return row[n]
    raise KeyError(names)


def load(path):
    files = [path] if os.path.isfile(path) else sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        sys.exit("no *kernel_trace.csv under %s" % path)
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                rows.append((int(_col(r, "Dispatch_Id", "Correlation_Id")), _col(r, "Kernel_Name").split("(")[0],
                             int(_col(r, "Start_Timestamp")), int(_col(r, "End_Timestamp"))))
    rows.sort()
    return rows


def union_len(iv):
    """Length of the union of the intervals iv (a list of (start, end))."""
    tot, end = 0, None
    for a, b in sorted(iv):
        if end is None or a > end:
            tot += b - a
            end = b
        elif b > end:
            tot += b - end
            end = b
    return tot


def covered(a, b, others):
    """Length of [a, b) covered by the union of `others` (sorted, merged intervals)."""
    tot = 0
    for c, d in others:
        if d <= a:
            continue
        if c >= b:
            break
        tot += min(b, d) - max(a, c)
    return tot


def merged(iv):
    out = []
    for a, b in sorted(iv):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("trace", help="rocprofv3's output directory, or its kernel_trace.csv")
    ap.add_argument("--skip", type=int, default=106, help="events left out at the start")
    ap.add_argument("--count", type=int, default=35, help="events looked at")
    ap.add_argument("--near", type=int, default=8, help="events before and after one that may overlap it")
    args = ap.parse_args()
    rows = load(args.trace)
    ev, events = -1, {}
    for _, name, t0, t1 in rows:
        if name == "k_event_init":
            ev += 1
        if ev >= 0:
            events.setdefault(ev, []).append((name, t0, t1))
    lo, hi = args.skip, min(args.skip + args.count, len(events))
    if hi - lo < 2:
        sys.exit("only %d events in the trace" % len(events))
    per = {}
    for e in range(lo, hi):
        near = [(t0, t1) for o in range(max(0, e - args.near), min(len(events), e + args.near + 1)) if o != e for _, t0, t1 in events[o]]
        others = merged(near)
        for name, t0, t1 in events[e]:
            same = merged([(a, b) for n2, a, b in events[e] if (n2, a, b) != (name, t0, t1)])
            anyk = merged([tuple(x) for x in others] + [tuple(x) for x in same])
            p = per.setdefault(name, [0, 0, 0, 0])
            p[0] += 1
            p[1] += t1 - t0
            p[2] += covered(t0, t1, others)
            p[3] += (t1 - t0) - covered(t0, t1, anyk)
    print("# events %d .. %d of %d in the trace" % (lo, hi - 1, len(events)))
    print("# %-28s %8s %10s %14s %8s" % ("kernel", "launches", "mean us", "other event %", "alone %"))
    for name, (n, dur, ov, alone) in sorted(per.items(), key=lambda kv: -kv[1][1]):
        if dur:
            print("  %-28s %8d %10.2f %14.1f %8.1f" % (name, n, dur / n / 1e3, 100.0 * ov / dur, 100.0 * alone / dur))
    allk = [(t0, t1) for e in range(lo, hi) for _, t0, t1 in events[e]]
    busy = union_len(allk)
    span = max(b for _, b in allk) - min(a for a, _ in allk)
    kernel_sum = sum(b - a for a, b in allk)
    print("# GPU busy (union of kernel intervals) %.3f ms per event; wall %.3f ms per event; sum of kernel durations %.3f ms per event"
          % (busy / 1e6 / (hi - lo), span / 1e6 / (hi - lo), kernel_sum / 1e6 / (hi - lo)))


if __name__ == "__main__":
    main()
