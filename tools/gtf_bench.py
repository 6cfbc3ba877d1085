#!/usr/bin/env python3
"""Times lesseq_amd.gencode.parse_gtf on a generated GENCODE-shaped GTF (needs a GPU):

    python tools/gtf_bench.py [--genes 60000] [--seed 1] [--keep PATH]

The default shape is 60 000 genes x 4 transcripts x 8 exons: 1 920 000 `exon` lines among 2 220 000, about 0.72 GB.  After
one warm-up call: wall clock of a call, the phases by HIP events (lsq_gtf_result_times) and, per phase, the bytes it has to
move at least -- the text read once per pass over it, the records written once -- over its time, against the HBM peak of
the MI355X.  The yardstick is the reference's own parseGencode on the same file: `tools/make_gtf_golden.py --time` takes
that figure where the reference is at hand.  One JSON line at the end."""
import argparse
import json
import os
import random
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_GBS = 8000.0          # MI355X: 8 TB/s


def generate(path, seed=1, genes=60000, transcripts=4, exons=8):
    """A GENCODE-shaped GTF: per gene a `gene` line, per transcript a `transcript` line and `exon` lines with a dozen
    attributes (gene lines carry a transcript_id, as GENCODE's did up to release 19: the reference asks every line for
    one).  Returns (lines, exon lines)."""
    rng = random.Random(seed)
    n_lines = n_exon = 0
    with open(path, "wb") as f:
        buf = []
        for g in range(genes):
            chrom = "chr%d" % (1 + g % 22)
            strand = "+-"[g & 1]
            gid = "ENSG%011d.%d" % (g, 1 + g % 9)
            gname = "GENE%d" % g
            base = 10000 + 40000 * (g // 22)
            common = 'gene_id "%s"; %%s gene_type "protein_coding"; gene_name "%s";' % (gid, gname)
            buf.append("%s\tHAVANA\tgene\t%d\t%d\t.\t%s\t.\t%s level 2;\n" % (chrom, base, base + 30000, strand, common % ('transcript_id "%s";' % gid)))
            n_lines += 1
            for t in range(transcripts):
                tid = "ENST%011d.%d" % (g * transcripts + t, 1 + t)
                tattr = common % ('transcript_id "%s";' % tid) + ' transcript_type "protein_coding"; transcript_name "%s-20%d";' % (gname, t)
                buf.append("%s\tHAVANA\ttranscript\t%d\t%d\t.\t%s\t.\t%s level 2; tag \"basic\";\n" % (chrom, base, base + 30000, strand, tattr))
                n_lines += 1
                pos = base + rng.randrange(0, 500)
                for x in range(exons):
                    length = rng.randrange(60, 400)
                    buf.append('%s\tHAVANA\texon\t%d\t%d\t.\t%s\t.\t%s exon_number %d; exon_id "ENSE%011d.1"; level 2; tag "basic"; tag "CCDS"; havana_gene "OTTHUMG%011d.2";\n'
                               % (chrom, pos, pos + length, strand, tattr, x + 1, (g * transcripts + t) * exons + x, g))
                    pos += length + rng.randrange(100, 3000)
                    n_lines += 1
                    n_exon += 1
            if len(buf) >= 4096:
                f.write("".join(buf).encode())
                buf = []
        f.write("".join(buf).encode())
    return n_lines, n_exon


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=60000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--keep", help="write the GTF here and keep it")
    ap.add_argument("--calls", type=int, default=3)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import lesseq_amd as L
    from lesseq_amd import gencode
    with tempfile.TemporaryDirectory() as d:
        path = a.keep or os.path.join(d, "bench.gtf")
        n_lines, n_exon = generate(path, a.seed, a.genes)
        size = os.path.getsize(path)
        ctx = L.Context(0)
        gencode.parse_gtf(ctx, path)                 # warm-up: code objects, the first touch of the file's pages
        best = None
        for _ in range(a.calls):
            ctx.synchronize()
            t0 = time.perf_counter()
            g = gencode.parse_gtf(ctx, path)
            ctx.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            if best is None or wall < best[0]:
                best = (wall, g.times_ms(), g.num_transcripts, g.num_exon_lines)
    wall, ms, n_tx, n_kept = best
    rec = 56
    # bytes a phase moves at least: the copy and the newline scan read the text once; the parse reads the text once, writes
    # a record per exon line, reads and writes them again to compact them; the download carries (start, end) per exon line
    # and a record per run head (about one per transcript)
    moved = [size, size, size + 3 * rec * n_kept + 8 * n_kept, 8 * n_kept + rec * n_tx]
    names = ["copy_to_hbm", "newline_scan", "parse_kernels", "download"]
    out = {"bytes": size, "lines": n_lines, "exon_lines": n_exon, "transcripts": n_tx, "wall_ms": round(wall, 3),
           "copy_share_of_device_ms": round(ms[0] / max(sum(ms), 1e-9), 3)}
    for n, t, b in zip(names, ms, moved):
        gbs = b / max(t, 1e-9) / 1e6
        out[n] = {"ms": round(t, 3), "min_bytes": b, "GB_per_s": round(gbs, 1)}
        if n in ("newline_scan", "parse_kernels"):
            out[n]["fraction_of_hbm_peak"] = round(gbs / HBM_PEAK_GBS, 4)
    assert n_kept == n_exon, (n_kept, n_exon)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
