#!/usr/bin/env python3
"""SAM_SINGLE against MRF_SINGLE through the loader chain on the GPU box: one read set written both ways, text in the page
cache -> pools in HBM, per pass.
    python tools/sam_bench.py [--reads N] [--events N] [--reps K] [--out FILE]
One process; its temporary directory is removed on every way out.  Prints (and writes to --out) one JSON object: per
format the text bytes, the copy to HBM (ms, GB/s), per pass of the chain the device milliseconds (HIP events on the
library's stream, lsq_last_ingest_stages), GB/s and reads/s, the from-text wall clock (stage + parse + ingest), and the
two figures DESIGN.md 4.9 discusses: the SAM routing pass over the newline-count pass on the same text, and over the MRF
routing pass on the same reads.  For the kernels' own times run it under `rocprofv3 --kernel-trace --stats -- python
tools/sam_bench.py ...` (no counters in that run)."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import lesseq_amd as L  # noqa: E402


def measure(ctx, path, fmt, n_reads, reps):
    size = os.path.getsize(path)
    runs = []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        text = ctx.stage_text(path)
        t1 = time.perf_counter()
        ctx.upload_reads_text(0, text, has_header=(fmt == "MRF_SINGLE"), first_line=1, read_format=fmt, free=True)
        t2 = time.perf_counter()
        st = ctx.ingest_stages()
        for s in st:
            s["GBps"] = (s["bytes"] / (s["ms"] * 1e-3) / 1e9) if s["ms"] > 0 else None
            s["reads_per_s"] = (n_reads / (s["ms"] * 1e-3)) if s["ms"] > 0 else None
        h2d = ctx.mrf_timing()["h2d_ms"]
        runs.append({"copy_ms": h2d, "copy_GBps": size / (h2d * 1e-3) / 1e9 if h2d > 0 else None, "stage_text_s": t1 - t0, "parse_and_ingest_s": t2 - t1,
                     "from_text_wall_s": t2 - t0, "copy_share_of_from_text": (t1 - t0) / (t2 - t0), "device_ms_total": sum(s["ms"] for s in st), "stages": st})
    best = min(runs, key=lambda r: r["device_ms_total"])
    return {"format": fmt, "text_bytes": size, "bytes_per_read": size / n_reads, "retained": ctx.retained(0), "runs": runs, "best": best}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000000)
    ap.add_argument("--events", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    d = tempfile.mkdtemp(prefix="lsq_sam_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        spec = L.SynthSpec(2027, a.events, a.reads, 100, 8, L.EVENT_TYPES, zipf=True)
        t0 = time.time()
        L.synth_write(spec, d, "s", write_mrf=True)
        t1 = time.time()
        L.synth_write_sam(spec, d, "s")
        t2 = time.time()
        ev = L.Events(L.Annotation(os.path.join(d, "s.interval"), os.path.join(d, "s.map"), 0, 10 ** 9), ("SHORT_READ",), (100,))
        ctx = L.Context(0)
        ctx.upload_events(ev)
        out = {"n_reads": a.reads, "n_events": a.events, "write_mrf_s": round(t1 - t0, 2), "write_sam_s": round(t2 - t1, 2)}
        out["mrf"] = measure(ctx, os.path.join(d, "s.mrf"), "MRF_SINGLE", a.reads, a.reps)
        ctx.count()
        out["mrf"]["valid_assignments"] = int(ctx.counts()[0].sum())
        out["sam"] = measure(ctx, os.path.join(d, "s.sam"), "SAM_SINGLE", a.reads, a.reps)
        out["sam"]["paths"] = ctx.sam_paths()
        ctx.count()
        out["sam"]["valid_assignments"] = int(ctx.counts()[0].sum())
        ctx.close()
        stage = lambda r, name: next(s for s in r["best"]["stages"] if s["stage"] == name)      # noqa: E731
        nl, route, mroute = stage(out["sam"], "newline_count"), stage(out["sam"], "sam_route"), stage(out["mrf"], "route")
        out["summary"] = {"sam_newline_count_ms": nl["ms"], "sam_newline_count_GBps": nl["GBps"], "sam_route_ms": route["ms"], "sam_route_GBps": route["GBps"],
                          "sam_route_over_newline_count": route["ms"] / nl["ms"] if nl["ms"] > 0 else None,
                          "mrf_route_ms": mroute["ms"], "sam_route_over_mrf_route": route["ms"] / mroute["ms"] if mroute["ms"] > 0 else None,
                          "sam_text_over_mrf_text": out["sam"]["text_bytes"] / out["mrf"]["text_bytes"],
                          "sam_copy_ms": out["sam"]["best"]["copy_ms"], "sam_copy_share_of_from_text": out["sam"]["best"]["copy_share_of_from_text"]}
        text = json.dumps(out, indent=1)
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text + "\n")
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
