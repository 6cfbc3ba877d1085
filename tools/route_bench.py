#!/usr/bin/env python3
"""The route pass of the loader per read format and library type on the GPU box (DESIGN 4.11's table).
    python tools/route_bench.py <package root> <library unstranded|forward|reverse> <reps> <data dir>
<package root>: the directory that holds the lesseq_amd package to measure ("." for this tree; another build's for an A/B run on
the same files).  The first run writes the data -- 4 M synthetic reads over 5 000 events on 24 chromosomes as MRF, SAM and BAM --
into <data dir>; later runs reuse it.  Prints one JSON line: per format the device milliseconds of the routing pass
(lsq_last_ingest_stages: "route", "sam_route", "bam_route") of <reps> uploads after one that warms up, and, for a stranded library,
the library report.  A developer aid, not a test; tools/ingest_bench.py gives every pass of the chain for MRF."""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pkg_root, library, reps, d = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]
sys.path.insert(0, pkg_root)
import lesseq_amd as L  # noqa: E402
assert os.path.abspath(L.__file__).startswith(os.path.abspath(pkg_root)), L.__file__
sys.path.insert(1, os.path.join(REPO, "tools"))
sys.path.insert(1, os.path.join(REPO, "tests"))

N_READS, N_EVENTS, RLEN, N_CHROM = 4_000_000, 5000, 100, 24
spec = L.SynthSpec(3, N_EVENTS, N_READS, RLEN, N_CHROM, L.EVENT_TYPES)
os.makedirs(d, exist_ok=True)
if not os.path.exists(os.path.join(d, "done")):
    t0 = time.time()
    L.synth_write(spec, d, "s", write_mrf=True)
    L.synth_write_sam(spec, d, "s")
    from bam_bench import write_bams
    write_bams(os.path.join(d, "s.sam"), os.path.join(d, "s.bam"), os.path.join(d, "s_cut.bam"))
    os.remove(os.path.join(d, "s_cut.bam"))
    open(os.path.join(d, "done"), "w").close()
    print("generated in %.1f s" % (time.time() - t0), file=sys.stderr)
ann = L.Annotation(os.path.join(d, "s.interval"), os.path.join(d, "s.map"), 0, 10 ** 9)
ev = L.Events(ann, ("SHORT_READ",), (RLEN,)) if library == "unstranded" else L.Events(ann, ("SHORT_READ",), (RLEN,), library=library)
ctx = L.Context(0)
ctx.upload_events(ev)
out = {"package": pkg_root, "library": library, "reads": N_READS, "bytes": {k: os.path.getsize(os.path.join(d, "s." + k)) for k in ("mrf", "sam", "bam")}}
for fmt, stage, up in (("mrf", "route", ctx.upload_reads_mrf), ("sam", "sam_route", ctx.upload_reads_sam), ("bam", "bam_route", ctx.upload_reads_bam)):
    ms = []
    for rep in range(reps + 1):
        up(0, os.path.join(d, "s." + fmt))
        st = {s["stage"]: s["ms"] for s in ctx.ingest_stages()}
        if rep:                      # (the first upload of a format warms the code and the page cache)
            ms.append(round(st[stage], 4))
    out[fmt] = {"route_ms": ms, "median": sorted(ms)[len(ms) // 2], "min": min(ms), "max": max(ms), "retained": ctx.retained(0)}
    if library != "unstranded":
        out[fmt]["report"] = list(ctx.library_report(0))
ctx.close()
print(json.dumps(out))
