#!/usr/bin/env python3
"""BAM_SINGLE against SAM_SINGLE through the loader chain on the GPU box: the generator's reads of tools/sam_bench.py's shape written
as SAM, and that SAM rewritten as BAM with Python's zlib (tests/bam_writer.py's records; at most 16 worker processes).  A developer
aid, not a test.
    python tools/bam_bench.py [--reads N] [--events N] [--reps K] [--verify] [--out FILE]
One run, one box, the files in the page cache.  Prints (and writes to --out) one JSON object:
  bam          the BAM as htslib lays it out (every block begins with a record): file bytes, the copy to HBM, per pass of the chain
               the device milliseconds (HIP events on the library's stream, lsq_last_ingest_stages), the from-file wall clock
               (stage + inflate + record starts + route + ingest)
  bam_cut      the same inflated stream cut every 0xff00 bytes regardless of records -- all but a worker's first block begin inside
               a record -- so that the repair pass walks nearly every block
  sam          the SAM text of the same reads through the SAM_SINGLE path (code this change leaves as it was), measured beside it
  host         one thread inflating the file: zlib (what a `samtools view` in front of the run pays), and the library's own decoder
               and parser (Reads.from_bam, n_threads=1)
  bam_verified (--verify) the htslib-layout BAM once more with the option "bam_verify" on -- the bgzf_crc32 pass beside the inflate of
               the same run, the from-file wall clock against the unverified one -- and, under host, one thread of zlib.crc32 over
               the same inflated bytes: what a check in front of the run costs
"""
import argparse
import json
import multiprocessing
import os
import shutil
import struct
import sys
import tempfile
import time
import zlib

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lesseq_amd as L  # noqa: E402
import bam_writer as bw  # noqa: E402

WORKERS = min(16, os.cpu_count() or 1)


def convert(job):
    """a run of SAM record lines -> (BGZF bytes with every block on a record, BGZF bytes cut every MAX_PAYLOAD bytes)"""
    lines, ids = job
    recs = [bw.record(ln.split("\t"), ids) for ln in lines]
    chunks, cur, n = [], [], 0
    for r in recs:
        if cur and n + len(r) > bw.MAX_PAYLOAD:
            chunks.append(b"".join(cur))
            cur, n = [], 0
        cur.append(r)
        n += len(r)
    if cur:
        chunks.append(b"".join(cur))
    stream = b"".join(recs)
    return b"".join(bw.bgzf_block(c) for c in chunks), b"".join(bw.bgzf_block(c) for c in bw.split_stream(stream, "htslib"))


def write_bams(sam_path, aligned_path, cut_path, lines_per_job=100000):
    with open(sam_path, "rb") as f:
        lines = f.read().decode("latin-1").split("\n")[:-1]
    n_head = 0
    while lines[n_head].startswith("@"):
        n_head += 1
    text, refs, _ = bw.parse_sam(("\n".join(lines[:n_head + 1]) + "\n").encode("latin-1"))
    names = [r[0] for r in refs]
    for ln in lines[n_head:]:
        rn = ln.split("\t", 3)[2]
        if rn != "*" and rn not in names:
            names.append(rn)
    ids = {nm: i for i, nm in enumerate(names)}
    t = text.encode("latin-1")
    head = b"BAM\x01" + struct.pack("<I", len(t)) + t + struct.pack("<I", len(names))
    for nm in names:
        b = nm.encode("latin-1") + b"\0"
        head += struct.pack("<I", len(b)) + b + struct.pack("<I", 0)
    jobs = [(lines[i:i + lines_per_job], ids) for i in range(n_head, len(lines), lines_per_job)]
    with multiprocessing.Pool(WORKERS) as pool, open(aligned_path, "wb") as fa, open(cut_path, "wb") as fc:
        fa.write(bw.bgzf_block(head))
        fc.write(bw.bgzf_block(head))
        for a, c in pool.imap(convert, jobs):
            fa.write(a)
            fc.write(c)
        fa.write(bw.EOF_BLOCK)
        fc.write(bw.EOF_BLOCK)
    return len(lines) - n_head


def measure(ctx, path, fmt, n_reads, reps):
    size = os.path.getsize(path)
    runs = []
    for _ in range(reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        text = ctx.stage_text(path)
        t1 = time.perf_counter()
        ctx.upload_reads_text(0, text, has_header=False, first_line=1, read_format=fmt, free=True)
        t2 = time.perf_counter()
        st = ctx.ingest_stages()
        for s in st:
            s["GBps"] = (s["bytes"] / (s["ms"] * 1e-3) / 1e9) if s["ms"] > 0 else None
        h2d = ctx.mrf_timing()["h2d_ms"]
        runs.append({"copy_ms": h2d, "stage_s": t1 - t0, "parse_and_ingest_s": t2 - t1, "from_file_wall_s": t2 - t0, "device_ms_total": sum(s["ms"] for s in st), "stages": st})
    best = min(runs, key=lambda r: r["from_file_wall_s"])
    return {"format": fmt, "file_bytes": size, "bytes_per_read": size / n_reads, "retained": ctx.retained(0), "runs": runs, "best": best}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000000)
    ap.add_argument("--events", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--verify", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    d = tempfile.mkdtemp(prefix="lsq_bam_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        spec = L.SynthSpec(2027, a.events, a.reads, 100, 8, L.EVENT_TYPES, zipf=True)
        L.synth_write_sam(spec, d, "s")
        sam, bam, cut = (os.path.join(d, n) for n in ("s.sam", "s.bam", "s.cut.bam"))
        t0 = time.time()
        n_rec = write_bams(sam, bam, cut)
        out = {"n_reads": a.reads, "n_records": n_rec, "n_events": a.events, "write_bams_s": round(time.time() - t0, 2), "workers": WORKERS}
        ev = L.Events(L.Annotation(os.path.join(d, "s.interval"), os.path.join(d, "s.map"), 0, 10 ** 9), ("SHORT_READ",), (100,))
        ctx = L.Context(0)
        ctx.upload_events(ev)
        tables = {}
        for key, path, fmt in (("sam", sam, "SAM_SINGLE"), ("bam", bam, "BAM_SINGLE"), ("bam_cut", cut, "BAM_SINGLE"), ("sam_again", sam, "SAM_SINGLE"), ("bam_again", bam, "BAM_SINGLE")):
            out[key] = measure(ctx, path, fmt, a.reads, a.reps)
            if fmt == "BAM_SINGLE":
                out[key]["paths"] = ctx.bam_paths()
            ctx.count()
            tables[key] = L.format_count(ev, ctx.counts()[0])
        if a.verify:
            ctx.set_option("bam_verify", 1)
            out["bam_verified"] = measure(ctx, bam, "BAM_SINGLE", a.reads, a.reps)
            ctx.set_option("bam_verify", 0)
            ctx.count()
            tables["bam_verified"] = L.format_count(ev, ctx.counts()[0])
        out["count_tables_equal"] = len(set(tables.values())) == 1
        ctx.close()
        with open(bam, "rb") as f:
            data = f.read()
        t0 = time.perf_counter()
        o, total, payloads = 0, 0, []
        while o < len(data):
            n = struct.unpack_from("<H", data, o + 16)[0] + 1
            payloads.append(zlib.decompress(data[o + 18:o + n - 8], -15))
            total += len(payloads[-1])
            o += n
        t1 = time.perf_counter()
        if not a.verify:
            payloads = []
        r = L.Reads.from_bam(bam, ev, n_threads=1)
        t2 = time.perf_counter()
        out["host"] = {"inflated_bytes": total, "zlib_one_thread_inflate_s": t1 - t0, "library_one_thread_inflate_and_parse_s": t2 - t1, "reads": len(r)}
        if a.verify:
            t3 = time.perf_counter()
            n_sums = len([zlib.crc32(p) for p in payloads])
            out["host"]["zlib_one_thread_crc32_s"] = time.perf_counter() - t3
            out["host"]["crc32_blocks"] = n_sums
        wall = lambda k: out[k]["best"]["from_file_wall_s"]      # noqa: E731
        out["summary"] = {"bam_from_file_ms": 1e3 * min(wall("bam"), wall("bam_again")), "sam_from_text_ms": 1e3 * min(wall("sam"), wall("sam_again")),
                          "bam_cut_from_file_ms": 1e3 * wall("bam_cut"), "bam_bytes_over_sam_bytes": out["bam"]["file_bytes"] / out["sam"]["file_bytes"],
                          "bam_stages_ms": {s["stage"]: s["ms"] for s in out["bam"]["best"]["stages"]},
                          "bam_cut_stages_ms": {s["stage"]: s["ms"] for s in out["bam_cut"]["best"]["stages"]},
                          "blocks": out["bam_cut"]["paths"]["blocks"], "blocks_repaired_in_cut_file": out["bam_cut"]["paths"]["blocks_repaired"]}
        if a.verify:
            v = out["bam_verified"]["best"]
            out["summary"]["verify"] = {"bgzf_crc32_ms": next(s["ms"] for s in v["stages"] if s["stage"] == "bgzf_crc32"),
                                        "bgzf_inflate_ms_same_run": next(s["ms"] for s in v["stages"] if s["stage"] == "bgzf_inflate"),
                                        "bgzf_crc32_GBps": next(s["GBps"] for s in v["stages"] if s["stage"] == "bgzf_crc32"),
                                        "from_file_ms_verified": 1e3 * v["from_file_wall_s"], "from_file_ms_unverified": out["summary"]["bam_from_file_ms"],
                                        "zlib_one_thread_crc32_ms": 1e3 * out["host"]["zlib_one_thread_crc32_s"], "inflated_bytes": total}
        text = json.dumps(out, indent=1)
        print(json.dumps(out["summary"], indent=1))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text + "\n")
        else:
            print(text)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
