#!/usr/bin/env python3
"""Junction and exon-body reads per event form of a read file on the GPU box (lsq_fe_device against the parse ahead of it, against
the psi count and the exon-bin count over the same file -- the kernel does the work of both lookups -- and against lsq_fe_host_reads):
    python tools/evidence_bench.py [--reads N] [--events N] [--reps K] [--step-timeout S] [--orders sorted,shuffled] [--library unstranded|forward|reverse] [--out FILE]
The generator's library (SynthSpec: --reads reads over --events events, Zipf depth, 8 chromosomes; the build of
tools/psi_bench.py) against the generator's own events, written coordinate-sorted and shuffled as MRF.  Every file's device run
is a child process of its own under `timeout`, and the first one that fails ends the run.  Per file: the report, the events, forms,
informative introns and regions; the device milliseconds of each phase (lsq_fe_table_times) beside the same run's copy and parse
(lsq_last_mrf_timing), every one of --reps calls and the best by the count phase; in the same process and on the same file the
phases of lsq_ps_device and of lsq_xb_device, --reps calls each; and lsq_fe_host_reads from already-parsed arrays on 1 and on 16
threads, its table compared with the device's.  --library: stranded counting in this tool's own index; the runs reported for comparison stay unstranded.  Prints one JSON object, and writes it to --out after every file.  At most 16 host
threads."""
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
    return hashlib.sha256(t.reads.tobytes() + t.total.tobytes()).hexdigest()[:16]


def child(a):
    import lesseq_amd as L
    ann = L.Annotation(a.interval, a.map)
    ix = L.EvidenceIndex(ann, a.library)
    ctx = L.Context(0)
    runs = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        t = ix.device(ctx, "MRF_SINGLE", a.reads_path)
        wall = time.perf_counter() - t0
        tm = ctx.mrf_timing()
        runs.append({"wall_s": wall, "copy_ms": tm["h2d_ms"], "parse_ms": tm["parse_ms"], "phases_ms": t.times})
    best = min(runs, key=lambda r: r["phases_ms"]["count"])
    out = {"text_bytes": os.path.getsize(a.reads_path), "report": t.report, "library_report": t.library_report() if a.library != "unstranded" else None, "events": ix.num_events, "forms": ix.num_forms, "introns": ix.num_introns, "regions": ix.num_regions,
           "largest_form": int(t.reads.max()) if len(t) else 0, "forms_hit": int((t.reads > 0).sum()), "psi_rows_not_na": int((t.psi(100) == t.psi(100)).sum()),
           "table_digest": digest(t), "best": best, "runs": runs}
    # the two counts whose lookups this one joins, behind the same parse, for the comparison
    px, xx = L.PsiIndex(ann), L.ExonBinIndex(ann)
    ps, xb = [], []
    for _ in range(a.reps):
        q = px.device(ctx, "MRF_SINGLE", a.reads_path)
        ps.append(dict(q.times, parse_ms=ctx.mrf_timing()["parse_ms"]))
        x = xx.device(ctx, "MRF_SINGLE", a.reads_path)
        xb.append(dict(x.times, parse_ms=ctx.mrf_timing()["parse_ms"]))
    out["psi_runs"], out["exonbins_runs"] = ps, xb
    out["psi_best"] = min(ps, key=lambda r: r["count"])
    out["exonbins_best"] = min(xb, key=lambda r: r["count"])
    out["psi_counted"], out["exonbins_bin_hits"] = q.report["counted"], x.report["bin_hits"]
    ctx.close()
    print("RESULT " + json.dumps(out))


def host_runs(L, d, stem, library):
    ix = L.EvidenceIndex(L.Annotation(os.path.join(d, stem + ".interval"), os.path.join(d, stem + ".map")), library)
    t0 = time.perf_counter()
    reads = ix.parse_host("MRF_SINGLE", os.path.join(d, stem + ".mrf"), n_threads=16)
    out = {"host_parse_16_threads_s": time.perf_counter() - t0}
    for nt in (1, 16):
        best = None
        for _ in range(2):
            t0 = time.perf_counter()
            t = ix.host_reads(reads, n_threads=nt)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        out["host_reads_%d_threads_s" % nt] = best
        out["table_digest"] = digest(t)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000000)
    ap.add_argument("--events", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--orders", default="sorted,shuffled")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--interval")
    ap.add_argument("--map")
    ap.add_argument("--reads-path")
    ap.add_argument("--library", default="unstranded", choices=("unstranded", "forward", "reverse"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    os.environ.setdefault("LSQ_NO_TORCH", "1")      # (the parent touches no GPU)
    import lesseq_amd as L
    d = tempfile.mkdtemp(prefix="lsq_fe_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = {"n_reads": a.reads, "n_events": a.events, "library": a.library, "files": []}

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
            argv = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--library", a.library,
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
            rec["host"] = host_runs(L, d, stem, a.library)
            rec["host_equals_device"] = rec["host"]["table_digest"] == rec["table_digest"]
            out["files"].append(rec)
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
