#!/usr/bin/env python3
"""from a rocprofv3 --kernel-trace --memory-copy-trace CSV directory: the hand-over of every chunk of work lists on its copy stream.
A chunk is the run of large host-to-device copies on one stream up to the prep_finish kernel that follows them there.  Per stream
and over all of them: copies per chunk, summed duration of the copies, summed gaps between consecutive copies, and the time from
the start of the first copy to the end of the last preparation kernel (medians over the chunks, microseconds) — are the copies
back to back, or does the stream stall between its commands?
Copy streams are the streams prep_finish runs on; a trace without a size column gives no bytes (MB and GB/s print as 0).
usage: trace_chunks.py <dir>"""
import csv, glob, os, sys
from collections import defaultdict

d = sys.argv[1]


def stream_of(r):
    for key in ("Stream_Id", "Queue_Id"):
        if r.get(key) not in (None, ""):
            return r[key]
    return "?"


ev = defaultdict(list)                     # stream -> (start, end, kind, bytes)
for fn in glob.glob(os.path.join(d, "**", "*memory_copy_trace.csv"), recursive=True):
    for r in csv.DictReader(open(fn)):
        if "DEVICE_TO_HOST" in r.get("Direction", "").upper():
            continue
        ev[stream_of(r)].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "copy", int(r.get("Size", r.get("Bytes", 0)) or 0)))
copy_streams = set()
for fn in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
    for r in csv.DictReader(open(fn)):
        name = r["Kernel_Name"].replace("void ", "")
        if name.startswith("prep_") or name.startswith("bs_kernel") or name.startswith("pull"):
            ev[stream_of(r)].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "finish" if name.startswith("prep_finish") else "prep", 0))
            if name.startswith("prep_finish"):
                copy_streams.add(stream_of(r))


def med(v):
    v = sorted(v)
    return v[len(v) // 2] if v else 0.0


print("stream   chunks  copies/chunk   MB/chunk   copies us   gaps us   first copy -> last prep us   GB/s while copying+gaps")
tot = []
for st in sorted(copy_streams):
    chunks, cur = [], []
    for s, e, kind, b in sorted(ev[st]):
        if kind == "copy":
            cur.append((s, e, b))
        elif kind == "finish" and cur:
            chunks.append((cur, e))
            cur = []
    rows = []
    for cp, fin in chunks:
        dur = sum(e - s for s, e, _ in cp)
        gaps = sum(max(0, cp[i + 1][0] - cp[i][1]) for i in range(len(cp) - 1))
        rows.append((len(cp), sum(b for _, _, b in cp), dur, gaps, fin - cp[0][0]))
    tot += rows
    if rows:
        print(f"{st:>6}  {len(rows):6d}  {med([r[0] for r in rows]):12.0f}  {med([r[1] for r in rows])/1e6:9.1f}  {med([r[2] for r in rows])/1e3:10.0f}"
              f"  {med([r[3] for r in rows])/1e3:8.0f}  {med([r[4] for r in rows])/1e3:26.0f}  {sum(r[1] for r in rows)/max(1, sum(r[2] + r[3] for r in rows)):8.1f}")
if tot:
    print(f"{'all':>6}  {len(tot):6d}  {med([r[0] for r in tot]):12.0f}  {med([r[1] for r in tot])/1e6:9.1f}  {med([r[2] for r in tot])/1e3:10.0f}"
          f"  {med([r[3] for r in tot])/1e3:8.0f}  {med([r[4] for r in tot])/1e3:26.0f}  {sum(r[1] for r in tot)/max(1, sum(r[2] + r[3] for r in tot)):8.1f}")
    print(f"share of the chunks' time on the copy stream (first copy -> last prep): copies {100*sum(r[2] for r in tot)/sum(r[4] for r in tot):.0f} %, "
          f"gaps between copies {100*sum(r[3] for r in tot)/sum(r[4] for r in tot):.0f} %")
