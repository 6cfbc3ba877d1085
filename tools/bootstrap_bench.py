#!/usr/bin/env python3
"""The read bootstrap on the GPU box (lsq_bootstrap behind a count and a solve of the benchmark's library):
    python tools/bootstrap_bench.py [--reads N] [--events N] [--replicates B] [--reps K] [--chunk N] [--step-timeout S] [--out FILE]
The generator's library of BASELINE configs[3]'s shape (bench.py's workload c3: --reads reads over --events mixed events, 24
chromosomes, seed 3) is made in memory, counted and solved once; then lsq_bootstrap runs --reps times with --replicates replicates
under lsq_set_timing, and the device milliseconds of its three phases -- resampling, EM, summaries, from HIP events
(lsq_debug_bootstrap_times) -- are reported for every run and for the best one, beside the wall time of the call, the counted
reads (the draws of one replicate) and the replicates per chunk.  The device run is a child process of its own under `timeout`.
Prints (and writes to --out) one JSON object.  At most 16 host threads."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def child(a):
    import numpy as np
    import lesseq_amd as L
    spec = L.SynthSpec(3, a.events, a.reads, 100, 24, L.EVENT_TYPES)
    ev = L.Events(L.Annotation(a.interval, a.map), ("SHORT_READ",), (100,))
    t0 = time.perf_counter()
    reads = L.Reads.synthetic(spec, ev, 16)
    make_s = time.perf_counter() - t0
    ctx = L.Context(0)
    if a.chunk:
        ctx.set_option("bootstrap_chunk", a.chunk)
    ctx.upload_events(ev)
    ctx.upload_reads(0, reads)
    ctx.set_timing(True)
    ctx.count(); ctx.solve()
    count_ms, solve_ms = ctx.timing()
    cnt, _ = ctx.counts()
    runs = []
    for k in range(a.reps):
        t0 = time.perf_counter()
        s = ctx.bootstrap(a.replicates, 1 + k)
        wall = time.perf_counter() - t0
        t = ctx.bootstrap_times()
        t["wall_ms"] = 1000 * wall
        t["total_device_ms"] = t["resample_ms"] + t["em_ms"] + t["summary_ms"]
        runs.append(t)
    best = min(runs, key=lambda r: r["total_device_ms"])
    ok = s["n_ok"] > 1
    out = {"events": len(ev), "isoforms": int(ev.total_isoforms), "classes": int(cnt.shape[1]), "host_genes": int(L.lib.lsq_events_host_genes(ev.h)),
           "counted_reads": int(cnt.sum()), "replicates": a.replicates, "make_reads_s": make_s, "count_ms": count_ms, "solve_ms": solve_ms,
           "best": best, "runs": runs, "isoforms_with_replicates": int(ok.sum()),
           "median_sd": float(np.median(s["sd"][ok])) if ok.any() else None,
           "median_interval_width": float(np.median((s["q975"] - s["q025"])[ok])) if ok.any() else None}
    ctx.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000000)
    ap.add_argument("--events", type=int, default=50000)
    ap.add_argument("--replicates", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--interval")
    ap.add_argument("--map")
    a = ap.parse_args()
    if a.child:
        return child(a)
    os.environ.setdefault("LSQ_NO_TORCH", "1")      # (the parent touches no GPU)
    import lesseq_amd as L
    with tempfile.TemporaryDirectory(prefix="lsq_boot_") as d:
        L.synth_write(L.SynthSpec(3, a.events, a.reads, 100, 24, L.EVENT_TYPES), d, "w", write_mrf=False)
        argv = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--reads", str(a.reads), "--events", str(a.events),
                "--replicates", str(a.replicates), "--reps", str(a.reps), "--chunk", str(a.chunk), "--interval", os.path.join(d, "w.interval"), "--map", os.path.join(d, "w.map")]
        env = dict(os.environ)
        env.pop("LSQ_NO_TORCH", None)
        p = subprocess.run(argv, capture_output=True, text=True, env=env)
        got = [ln for ln in p.stdout.split("\n") if ln.startswith("RESULT ")]
        out = {"n_reads": a.reads, "n_events": a.events, "exit": p.returncode}
        if p.returncode != 0 or not got:
            out["stderr_tail"] = p.stderr[-2000:]
        else:
            out.update(json.loads(got[0][7:]))
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if out["exit"] == 0 and "best" in out else 1


if __name__ == "__main__":
    sys.exit(main())
