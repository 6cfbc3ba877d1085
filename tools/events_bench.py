#!/usr/bin/env python3
"""Local events (bin/Events.r) at genome scale: a deterministic set of ~60 k genes / ~250 k transcripts (K up to 200,
N up to ~600, every event shape planted; tests/localev_ref.py), timed phase by phase, best of 3:

  annotation load + classify in memory   lsq_le_load_annotation (host)
  matrix load                            lsq_le_load_matrices over classify's files (host)
  upload / kernels / download            HIP events inside lsq_le_detect
  detect                                 lsq_le_detect, wall clock
  format + write                         lsq_le_write (host)
  CLI, both modes                        lesseq_amd/bin/events as a process, end to end

    python tools/events_bench.py [--genes 60000] [--json out.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lesseq_amd as L  # noqa: E402
from lesseq_amd import localevents as le  # noqa: E402
import localev_ref as R  # noqa: E402

BIN = os.path.join(ROOT, "lesseq_amd", "bin")


def best(f, n=3):
    ts, out = [], None
    for _ in range(n):
        t = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t)
    return min(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=60000)
    ap.add_argument("--json")
    a = ap.parse_args()
    res = {}
    with tempfile.TemporaryDirectory() as d:
        t = time.perf_counter()
        genes = R.gene_models(a.genes, seed=2026, wide_every=300, wide_shapes=((80, 20), (8, 70), (300, 200)))
        iv, mp = R.write_models(genes, d, "gen")
        res["generate_s"] = time.perf_counter() - t
        res["genes"], res["transcripts"] = len(genes), sum(len(x[1]) for x in genes)
        cls = os.path.join(d, "cls")
        os.makedirs(cls)
        rc, _ = L.cli_run("classify", ["0", "x", cls + "/", "LH_GENE_TXT", iv, "UCSC_GENE2ISOFORM", mp, "0", "100000000"])
        assert rc == 0
        res["annotation_classify_s"], g = best(lambda: le.Graphs.from_annotation(iv, mp))
        res["matrix_load_s"], g2 = best(lambda: le.Graphs.from_matrices(cls + "/", mp))
        shapes = [g.shape(i) for i in range(len(g))]
        res["max_N"], res["max_K"] = max(s[0] for s in shapes), max(s[1] for s in shapes)
        ctx = L.Context(0)
        g.detect(ctx)                                      # warm-up (code objects, allocator)
        res["detect_s"], r = best(lambda: g.detect(ctx))
        times = [r.times_ms()]
        for _ in range(2):
            times.append(g.detect(ctx).times_ms())
        ms = [min(x[q] for x in times) for q in range(4)]
        res["upload_ms"], res["count_scan_ms"], res["emit_ms"], res["download_ms"] = ms
        res["events"] = {t: r.num_events(t) for t in le.TYPES}

        def write():
            o = os.path.join(d, "w%d" % time.perf_counter_ns())
            os.makedirs(o)
            r.write(o + "/ev_")
        res["format_write_s"], _ = best(write)

        def cli(args):
            o = os.path.join(d, "c%d" % time.perf_counter_ns())
            os.makedirs(o)
            p = subprocess.run([os.path.join(BIN, "events")] + args + [o + "/ev_"], capture_output=True, timeout=600)
            assert p.returncode == 0, p.stderr[-2000:]
        res["cli_dropin_s"], _ = best(lambda: cli([cls + "/", mp]))
        res["cli_annotation_s"], _ = best(lambda: cli(["--annotation", "LH_GENE_TXT", iv, "UCSC_GENE2ISOFORM", mp]))
        ctx.close()
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
