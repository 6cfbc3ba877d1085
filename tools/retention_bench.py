#!/usr/bin/env python3
"""Intron retention of a read file on the GPU box (lsq_ir_device phase by phase, against the parse ahead of it, against sites and
coverage over the same file in the same session -- the sites phase is lsq_ss_device's four, the depth phase lsq_cov_device's first
four, and the selection's nearest kin are coverage's regions phase and sites' through phase -- and against lsq_ir_host_reads):
    python tools/retention_bench.py [--reads N] [--events N] [--reps K] [--step-timeout S] [--orders sorted,shuffled] [--out FILE]
The library of tools/exonbins_bench.py (SynthSpec: --reads reads over --events events, Zipf depth, 8 chromosomes) against its own
annotation, written coordinate-sorted and shuffled as MRF.  Every file's device run is a child process of its own under `timeout`,
and the first one that fails ends the run.  Per file: the report and the rows; the device milliseconds of each phase
(lsq_ir_table_times) beside the same run's copy and parse (lsq_last_mrf_timing), every one of --reps calls and the best by the
select phase; in the same process and on the same file the phases of lsq_ss_device and of lsq_cov_device, --reps calls each; and
lsq_ir_host_reads from already-parsed arrays on 16 threads (--host-threads: others as well), its table compared with the device's.
Prints one JSON object, and writes it to --out after every file.  At most 16 host threads."""
import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def digest(t):
    from lesseq_amd.retention import COLUMNS
    return hashlib.sha256(b"".join(getattr(t, k).tobytes() for k, _ in COLUMNS)).hexdigest()[:16]


def child(a):
    import numpy as np
    import lesseq_amd as L
    ann = L.Annotation(a.interval, a.map)
    ix = L.RetentionIndex(ann)
    ctx = L.Context(0)
    runs = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        t = ix.device(ctx, "MRF_SINGLE", a.reads_path)
        wall = time.perf_counter() - t0
        tm = ctx.mrf_timing()
        runs.append({"wall_s": wall, "copy_ms": tm["h2d_ms"], "parse_ms": tm["parse_ms"], "phases_ms": t.times})
    best = min(runs, key=lambda r: r["phases_ms"]["select"])
    n = len(t)
    out = {"text_bytes": os.path.getsize(a.reads_path), "report": t.report, "rows": n, "introns": ix.num_introns, "table_digest": digest(t), "best": best, "runs": runs}
    if n:
        longest = int(np.argmax(t.clean))
        out.update(largest_clean=int(t.clean.max()), largest_q75=int(t.q75.max()), largest_q50=int(t.q50.max()), rows_covered=int((t.covered > 0).sum()),
                   rows_q50_positive=int((t.q50 > 0).sum()), clean_bases=int(t.clean.sum()), covered_bases=int(t.covered.sum()),
                   longest_intron={k: int(getattr(t, k)[longest]) for k in ("clean", "covered", "depth_sum", "q25", "q50", "q75")})
    # the tools whose passes this one runs, behind the same parse, for the comparison
    sx, cx = L.SiteIndex(ann), L.CoverageIndex(ann)
    ss, cv = [], []
    for _ in range(a.reps):
        s = sx.device(ctx, "MRF_SINGLE", a.reads_path)
        ss.append(dict(s.times, parse_ms=ctx.mrf_timing()["parse_ms"]))
        c = cx.device(ctx, "MRF_SINGLE", a.reads_path)
        cv.append(dict(c.times, parse_ms=ctx.mrf_timing()["parse_ms"]))
    out["sites_runs"], out["coverage_runs"] = ss, cv
    out["sites_best"] = min(ss, key=lambda r: r["through"])
    out["coverage_best"] = min(cv, key=lambda r: sum(r[k] for k in L.coverage.PHASES[:4]))
    out["coverage_rows"], out["coverage_regions"], out["sites_rows"] = len(c), cx.num_regions, len(s)
    ctx.close()
    print("RESULT " + json.dumps(out))


def host_runs(L, d, stem, threads):
    ix = L.RetentionIndex(L.Annotation(os.path.join(d, stem + ".interval"), os.path.join(d, stem + ".map")))
    t0 = time.perf_counter()
    reads = ix.parse_host("MRF_SINGLE", os.path.join(d, stem + ".mrf"), n_threads=16)
    out = {"host_parse_16_threads_s": time.perf_counter() - t0}
    for nt in threads:
        t0 = time.perf_counter()
        t = ix.host_reads(reads, n_threads=nt)
        out["host_reads_%d_threads_s" % nt] = time.perf_counter() - t0
        out["table_digest"] = digest(t)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000000)
    ap.add_argument("--events", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--orders", default="sorted,shuffled")
    ap.add_argument("--host-threads", default="16")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--interval")
    ap.add_argument("--map")
    ap.add_argument("--reads-path")
    a = ap.parse_args()
    if a.child:
        return child(a)
    os.environ.setdefault("LSQ_NO_TORCH", "1")      # (the parent touches no GPU)
    import lesseq_amd as L
    d = tempfile.mkdtemp(prefix="lsq_ir_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = {"n_reads": a.reads, "n_events": a.events, "files": []}

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
    try:
        ok = True
        for order in a.orders.split(","):
            stem = "%s_mrf" % order
            spec = L.SynthSpec(2027, a.events, a.reads, 100, 8, L.EVENT_TYPES, zipf=True, sorted_reads=(order == "sorted"))
            t0 = time.time()
            L.synth_write(spec, d, stem, write_mrf=True)
            path = os.path.join(d, stem + ".mrf")
            rec = {"order": order, "n_reads": a.reads, "write_s": round(time.time() - t0, 2)}
            print("written %s" % order, file=sys.stderr, flush=True)
            argv = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps),
                    "--interval", os.path.join(d, stem + ".interval"), "--map", os.path.join(d, stem + ".map"), "--reads-path", path]
            env = dict(os.environ)
            env.pop("LSQ_NO_TORCH", None)
            p = subprocess.run(argv, capture_output=True, text=True, env=env)
            rec["exit"] = p.returncode
            got = [ln for ln in p.stdout.split("\n") if ln.startswith("RESULT ")]
            if p.returncode != 0 or not got:      # (a device step failed or ran out of time: nothing more is started on the GPU)
                rec["stderr_tail"] = p.stderr[-2000:]
                out["files"].append(rec)
                ok = False
                break
            rec.update(json.loads(got[0][7:]))
            print("device runs done %s" % order, file=sys.stderr, flush=True)
            out["files"].append(rec)
            save()
            rec["host"] = host_runs(L, d, stem, [int(v) for v in a.host_threads.split(",") if v])
            rec["host_equals_device"] = rec["host"]["table_digest"] == rec["table_digest"]
            os.remove(path)
            save()
            print("done %s" % order, file=sys.stderr, flush=True)
        save()
        print(json.dumps(out, indent=1))
        return 0 if ok else 1
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
