#!/usr/bin/env python3
"""Intron clusters on the GPU box (lsq_cl_device phase by phase, against lsq_cl_host on 1 and on 16 threads and against the
junction passes that make every sample's rows):
    python tools/clusters_bench.py [--samples K] [--reads N] [--events N] [--reps R] [--step-timeout S] [--pool-samples 64] [--out FILE]
K samples of one library: the generator's annotation of one seed (SynthSpec: --events events -- 300 000, about as many junction rows a sample --, Zipf depth, 8 chromosomes), sample k
its reads k N .. (k + 1) N, written as MRF one after another.  The device work is one child process under `timeout`; if it fails
nothing more is started on the GPU.  In the child: every file through lsq_jn_device (its phases and the parse ahead of them), the
tables pooled, lsq_cl_device --reps times (every call's phases and rounds, and the best by the sum), lsq_cl_host on 1 and on 16
threads with its table compared to the device's; then a synthetic pool of --pool-samples samples -- the first sample's rows, each
sample keeping 9 rows in 10 with reads drawn again (Poisson around the row's) -- through the same three.  Prints one JSON object and
writes it to --out.  At most 16 host threads."""
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
ARRAYS = ("chrom", "start", "end", "ann", "reads", "samples", "cluster", "status", "counts")


def digest(t):
    return hashlib.sha256(b"".join(getattr(t, k).tobytes() for k in ARRAYS)).hexdigest()[:16]


def solve_all(L, pool, ctx, reps, threads):
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        t = pool.device(ctx)
        runs.append({"wall_s": time.perf_counter() - t0, "phases_ms": t.times, "rounds": t.rounds})
    best = min(runs, key=lambda r: sum(r["phases_ms"].values()))
    out = {"samples": pool.num_samples, "pooled_rows": pool.num_rows, "report": t.report, "table_digest": digest(t), "runs": runs, "best": best,
           "largest_phase": max(best["phases_ms"], key=best["phases_ms"].get), "device_ms": sum(best["phases_ms"].values()), "host": {}}
    for nt in threads:
        t0 = time.perf_counter()
        h = pool.host(n_threads=nt)
        out["host"]["%d_threads_s" % nt] = time.perf_counter() - t0
        out["host_equals_device"] = out.get("host_equals_device", True) and digest(h) == out["table_digest"]
    return out


def child(a):
    import numpy as np
    import lesseq_amd as L
    ix = L.JunctionIndex(L.Annotation(a.interval, a.map))
    ctx = L.Context(0)
    pool = L.ClusterPool(ix)
    files, first = [], None
    for path in a.reads_paths.split(","):
        t0 = time.perf_counter()
        jt = ix.device(ctx, "MRF_SINGLE", path)
        wall = time.perf_counter() - t0
        tm = ctx.mrf_timing()
        files.append({"text_bytes": os.path.getsize(path), "rows": len(jt), "wall_s": wall, "copy_ms": tm["h2d_ms"], "parse_ms": tm["parse_ms"], "junction_phases_ms": jt.times})
        pool.add(jt)
        first = first if first is not None else jt
    threads = [int(v) for v in a.host_threads.split(",") if v]
    out = {"files": files, "generated": solve_all(L, pool, ctx, a.reps, threads)}
    rng = np.random.default_rng(5)
    big = L.ClusterPool(ix)
    for _ in range(a.pool_samples):
        keep = rng.random(len(first)) < 0.9
        big.add_rows(first.chrom[keep], first.start[keep], first.end[keep], rng.poisson(first.reads[keep]).astype(np.uint32))
    out["synthetic"] = solve_all(L, big, ctx, a.reps, threads)
    ctx.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--reads", type=int, default=10000000)
    ap.add_argument("--events", type=int, default=300000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pool-samples", type=int, default=64)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--host-threads", default="1,16")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--interval")
    ap.add_argument("--map")
    ap.add_argument("--reads-paths")
    a = ap.parse_args()
    if a.child:
        return child(a)
    os.environ.setdefault("LSQ_NO_TORCH", "1")      # (the parent touches no GPU)
    import lesseq_amd as L
    d = tempfile.mkdtemp(prefix="lsq_cl_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    out = {"n_samples": a.samples, "n_reads": a.reads, "n_events": a.events}
    try:
        paths = []
        t0 = time.time()
        for k in range(a.samples):
            stem = "s%d" % k
            L.synth_write(L.SynthSpec(2027, a.events, a.reads, 100, 8, L.EVENT_TYPES, zipf=True, first_read=k * a.reads, sorted_reads=True), d, stem, write_mrf=True)
            paths.append(os.path.join(d, stem + ".mrf"))
            print("written sample %d" % k, file=sys.stderr, flush=True)
        out["write_s"] = round(time.time() - t0, 2)
        argv = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--pool-samples", str(a.pool_samples),
                "--host-threads", a.host_threads, "--interval", os.path.join(d, "s0.interval"), "--map", os.path.join(d, "s0.map"), "--reads-paths", ",".join(paths)]
        env = dict(os.environ)
        env.pop("LSQ_NO_TORCH", None)
        p = subprocess.run(argv, capture_output=True, text=True, env=env)
        out["exit"] = p.returncode
        got = [ln for ln in p.stdout.split("\n") if ln.startswith("RESULT ")]
        if p.returncode != 0 or not got:
            out["stderr_tail"] = p.stderr[-2000:]
        else:
            out.update(json.loads(got[0][7:]))
        text = json.dumps(out, indent=1)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text + "\n")
        print(text)
        return 0 if p.returncode == 0 and got else 1
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
