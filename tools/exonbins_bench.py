#!/usr/bin/env python3
"""Reads per exon bin and per gene of a read file on the GPU box (lsq_xb_device against the parse ahead of it and against
lsq_xb_host_reads):
    python tools/exonbins_bench.py [--reads N] [--sam-reads N] [--events N] [--reps K] [--step-timeout S] [--orders sorted,shuffled] [--library unstranded|forward|reverse]
                                   [--formats MRF_SINGLE,SAM_SINGLE] [--out FILE]
The generator's library (SynthSpec: --reads reads over --events events, Zipf depth, 8 chromosomes) against its own gene annotation,
written coordinate-sorted and shuffled, as MRF and as SAM (--sam-reads: a SAM text is seven times its MRF text; default: --reads,
or what half of the free room of the temporary directory holds).  Every file's device run is a child process of its own under
`timeout`, and the first one that fails ends the run (--orders / --formats: a part of the files, for a run under a time limit).
Per file: the report, the bins and the genes; the device milliseconds of each phase (lsq_xb_table_times) beside the same run's copy
and parse (lsq_last_mrf_timing), best of --reps by the count phase; the peak of the device's used memory during the call, sampled;
and, for the MRF files, lsq_xb_host_reads from already-parsed arrays on 1 and on 16 threads, its table compared with the device's.
--library: stranded counting in this tool's own index; the runs reported for comparison stay unstranded.  Prints one JSON object, and writes it to --out after every file.  At most 16 host threads."""
import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import threading
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def digest(t):
    return hashlib.sha256(t.reads.tobytes() + t.total.tobytes()).hexdigest()[:16]


def child(a):
    import torch
    import lesseq_amd as L
    ix = L.ExonBinIndex(L.Annotation(a.interval, a.map), a.library)
    ctx = L.Context(0)
    free0 = torch.cuda.mem_get_info(0)[0]
    low = [free0]
    stop = threading.Event()

    def sample():
        while not stop.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info(0)[0])
            time.sleep(0.002)
    th = threading.Thread(target=sample)
    th.start()
    runs = []
    try:
        for _ in range(a.reps):
            t0 = time.perf_counter()
            t = ix.device(ctx, a.child, a.reads_path)
            wall = time.perf_counter() - t0
            tm = ctx.mrf_timing()
            runs.append({"wall_s": wall, "copy_ms": tm["h2d_ms"], "parse_ms": tm["parse_ms"], "phases_ms": t.times})
    finally:
        stop.set()
        th.join()
    best = min(runs, key=lambda r: r["phases_ms"]["count"])
    out = {"format": a.child, "text_bytes": os.path.getsize(a.reads_path), "report": t.report, "library_report": t.library_report() if a.library != "unstranded" else None, "bins": ix.num_bins, "genes": ix.num_genes,
           "largest_bin": int(t.reads.max()) if len(t) else 0, "largest_gene": int(t.total.max()) if len(t.total) else 0, "bins_hit": int((t.reads > 0).sum()),
           "sums_agree": int(t.reads.sum()) == t.report["bin_hits"], "table_digest": digest(t), "best": best, "runs": runs, "peak_device_bytes_sampled": free0 - low[0]}
    ctx.close()
    print("RESULT " + json.dumps(out))


def host_runs(L, d, stem, library):
    ix = L.ExonBinIndex(L.Annotation(os.path.join(d, stem + ".interval"), os.path.join(d, stem + ".map")), library)
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
    ap.add_argument("--sam-reads", type=int, default=None)
    ap.add_argument("--events", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--orders", default="sorted,shuffled")
    ap.add_argument("--formats", default="MRF_SINGLE,SAM_SINGLE")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--interval")
    ap.add_argument("--map")
    ap.add_argument("--reads-path")
    ap.add_argument("--library", default="unstranded", choices=("unstranded", "forward", "reverse"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    os.environ.setdefault("LSQ_NO_TORCH", "1")      # (the parent touches no GPU)
    import lesseq_amd as L
    d = tempfile.mkdtemp(prefix="lsq_xb_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = {"n_reads": a.reads, "n_events": a.events, "library": a.library, "files": []}

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
    try:
        sam_reads = a.sam_reads
        if sam_reads is None:
            room = shutil.disk_usage(d).free // 2 - 2 * 40 * a.reads
            sam_reads = max(min(a.reads, room // 260), 1000000)
        out["sam_reads"] = sam_reads
        ok = True
        for fmt in a.formats.split(","):
            n = a.reads if fmt == "MRF_SINGLE" else sam_reads
            for order in a.orders.split(","):
                stem = "%s_%s" % (order, fmt[:3].lower())
                spec = L.SynthSpec(2027, a.events, n, 100, 8, L.EVENT_TYPES, zipf=True, sorted_reads=(order == "sorted"))
                t0 = time.time()
                if fmt == "MRF_SINGLE":
                    L.synth_write(spec, d, stem, write_mrf=True)
                else:
                    L.synth_write_sam(spec, d, stem)
                path = os.path.join(d, stem + (".mrf" if fmt == "MRF_SINGLE" else ".sam"))
                rec = {"order": order, "format": fmt, "n_reads": n, "write_s": round(time.time() - t0, 2)}
                print("written %s %s" % (order, fmt), file=sys.stderr, flush=True)
                argv = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", fmt, "--reps", str(a.reps), "--library", a.library,
                        "--interval", os.path.join(d, stem + ".interval"), "--map", os.path.join(d, stem + ".map"), "--reads-path", path]
                env = dict(os.environ)
                env.pop("LSQ_NO_TORCH", None)
                p = subprocess.run(argv, capture_output=True, text=True, env=env)
                rec["exit"] = p.returncode
                got = [ln for ln in p.stdout.split("\n") if ln.startswith("RESULT ")]
                if p.returncode != 0 or not got:
                    rec["stderr_tail"] = p.stderr[-2000:]
                    out["files"].append(rec)
                    ok = False
                    break
                rec.update(json.loads(got[0][7:]))
                print("device runs done %s %s" % (order, fmt), file=sys.stderr, flush=True)
                save()
                if fmt == "MRF_SINGLE":
                    rec["host"] = host_runs(L, d, stem, a.library)
                    rec["host_equals_device"] = rec["host"]["table_digest"] == rec["table_digest"]
                out["files"].append(rec)
                os.remove(path)
                save()
                print("done %s %s" % (order, fmt), file=sys.stderr, flush=True)
            if not ok:      # (a device step failed or ran out of time: nothing more is started on the GPU)
                break
        save()
        print(json.dumps(out, indent=1))
        return 0 if ok else 1
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
