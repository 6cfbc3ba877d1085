#!/usr/bin/env python3
"""Developer aid: what holds a count back in the pipelined step, from a `rocprofv3 --kernel-trace --output-format csv` run of
`python bench.py --steps N --warmup W` (one fill per lsq_count: the zeroing of the counter set of the count before).
usage: python tools/counter_sets_trace.py <trace dir> [steady-state launches to use, default 40]
Prints, over the last launches of the timed loop: D (a count launch's duration), P (start to start), the overlap of consecutive
counts (a), the wait of count k+1 behind the fill that run_count(k) queued (b), the same behind the fill that run_count(k-1) queued
(three counter sets), start(k+1) - end(k-1), and an excerpt of the launches themselves."""
import csv, glob, os, sys

d = sys.argv[1]
n_use = int(sys.argv[2]) if len(sys.argv) > 2 else 40
rows = []
for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
    for r in csv.DictReader(open(f)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "%s/%s" % (r.get("Queue_Id", "?"), r.get("Stream_Id", "?")), r["Kernel_Name"]))
rows.sort()
if not rows:
    sys.exit("no kernel_trace.csv under %s" % d)
short = lambda n: n.replace("void ", "").replace("lsq::", "").replace("(anonymous namespace)::", "").split("(")[0]
counts = [r for r in rows if "lsq_count_fast_kernel" in r[3]]
fills = [r for r in rows if "fillBuffer" in r[3]]
n_use = min(n_use, len(counts) - 4)
# the last count of the run is the last run_count, and so is the last fill: index both from the end
cs, fs = counts[-(n_use + 3):], fills[-(n_use + 3):]
us = lambda t: t / 1e3


def stat(name, v):
    v = sorted(v)
    print("%-58s median %7.1f  min %7.1f  max %7.1f us  (n=%d)" % (name, v[len(v) // 2], v[0], v[-1], len(v)))


stat("D   = end(count k) - start(count k)", [us(c[1] - c[0]) for c in cs[3:]])
stat("P   = start(count k+1) - start(count k)", [us(cs[i + 1][0] - cs[i][0]) for i in range(2, len(cs) - 1)])
stat("(a) = end(count k) - start(count k+1)", [us(cs[i][1] - cs[i + 1][0]) for i in range(2, len(cs) - 1)])
stat("(b) = start(count k+1) - end(fill queued by run_count k)", [us(cs[i + 1][0] - fs[i][1]) for i in range(2, len(cs) - 1)])
for q in sorted(set(c[2] for c in cs)):
    stat("(b) for the counts on queue/stream %s" % q, [us(cs[i + 1][0] - fs[i][1]) for i in range(2, len(cs) - 1) if cs[i + 1][2] == q])
stat("      start(count k+1) - end(fill queued by run_count k-1)", [us(cs[i + 1][0] - fs[i - 1][1]) for i in range(2, len(cs) - 1)])
stat("      start(count k+1) - end(count k-1)", [us(cs[i + 1][0] - cs[i - 1][1]) for i in range(2, len(cs) - 1)])
t0, t1 = cs[-8][0], cs[-4][1]
print("\nexcerpt: the launches between the start of count N-8 and the end of count N-4, us from the former")
print("%10s %10s %9s  %-5s %s" % ("start", "end", "duration", "queue/stream", "kernel"))
for r in rows:
    if r[0] >= t0 and r[0] <= t1:
        print("%10.1f %10.1f %9.1f  %-5s %s" % (us(r[0] - t0), us(r[1] - t0), us(r[1] - r[0]), r[2], short(r[3])))
