#!/usr/bin/env python3
"""Capture tests/golden/wide/: gene models past classify's old 64-segment limit, and the .matrix files that the
reference's own classify writes for them.  CPU only, run in a build tree that has the reference next to it:

    make -C oracle ref && python tools/make_wide_golden.py

Genes (UCSC_GENE2ISOFORM ids, byte order: MANY, MINUS, SE, SOLO, WIDE):
  WIDE   + strand, 40 isoforms over 90 exons: N > 64 atomic segments (two words per row of masks); planted skipped
         exons, a retained intron and alternative 5' / 3' ends
  MANY   - strand, 70 isoforms: K > 64 (two words per column of the device packing); alternative first exons and a
         mutually exclusive pair
  MINUS  - strand: a skipped exon and an alternative start that abuts the next segment (T3 on -)
  SE     + strand: one ordinary skipped exon
  SOLO   one isoform (classify writes no matrix for it)
Nothing of the reference is copied: the inputs are invented here, the outputs are what its classify printed.
"""
import json
import os
import random
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "wide")
REF = os.environ.get("LSQ_REFERENCE", "/root/reference")


def interval_line(name, chrom, strand, exons):
    exons = sorted(exons)
    return "%s\t%s\t%s\t%d\t%d\t%d\t%s\t%s\n" % (name, chrom, strand, exons[0][0], exons[-1][1], len(exons),
                                              ",".join(str(s) for s, _ in exons), ",".join(str(e) for _, e in exons))


def genes():
    rng = random.Random(20261016)
    out = []          # (gene, isoform, chrom, strand, exons)
    # WIDE: exon j = [10000 + 300 j, +100); every isoform holds the first and last exon
    base = [(10000 + 300 * j, 10100 + 300 * j) for j in range(90)]
    for k in range(40):
        ex = list(base)
        if k < 20:
            del ex[2 + 4 * k]                              # one skipped exon each, constitutive neighbours
        elif k < 25:
            j = 3 + 4 * (k - 20) + 1                       # alternative 5' / 3' ends: abutting segments
            s, e = ex[j]
            ex[j] = (s, e + 30) if k % 2 else (s - 30, e)
        elif k == 25:
            s, _ = ex[60]
            _, e = ex[61]
            ex[60:62] = [(s, e)]                           # a retained intron
        else:
            for _ in range(rng.randint(1, 4)):             # random skips
                j = rng.randrange(1, len(ex) - 1)
                del ex[j]
        out.append(("WIDE", "WIDE.%d" % k, "chr1", "+", ex))
    # MANY: alternative first exons A0 / A1 (one each), C always, mutually exclusive M1 / M2, D always
    A0, A1, Cc, M1, M2, D = (500000, 500100), (500300, 500400), (500700, 500800), (501000, 501100), (501300, 501400), (501700, 501800)
    for k in range(70):
        ex = [A0 if k % 2 == 0 else A1, Cc, M1 if k % 3 == 0 else M2, D]
        if k % 7 == 0:
            ex.append((502000, 502100))                    # a last exon that only some isoforms hold
        out.append(("MANY", "MANY.%02d" % k, "chr2", "-", ex))
    out.append(("MINUS", "MINUS.a", "chr3", "-", [(1000, 1200), (1500, 1600), (2000, 2100)]))
    out.append(("MINUS", "MINUS.b", "chr3", "-", [(1050, 1200), (1500, 1600), (2000, 2100)]))
    out.append(("MINUS", "MINUS.c", "chr3", "-", [(1050, 1200), (2000, 2100)]))
    out.append(("SE", "SE.inc", "chr3", "+", [(9000, 9100), (9200, 9300), (9500, 9600)]))
    out.append(("SE", "SE.skp", "chr3", "+", [(9000, 9100), (9500, 9600)]))
    out.append(("SOLO", "SOLO.1", "chr4", "+", [(100, 200), (300, 400)]))
    return out


def main():
    if not os.path.isdir(os.path.join(ROOT, "oracle", "_ref", "lib")):
        sys.exit("run `make -C oracle ref` first")
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(os.path.join(OUT, "classify"))
    g = genes()
    with open(os.path.join(OUT, "wide.interval"), "w") as f:
        f.writelines(interval_line(i, c, s, ex) for _, i, c, s, ex in g)
    with open(os.path.join(OUT, "wide.map"), "w") as f:
        f.writelines("%s\t%s\n" % (gn, i) for gn, i, _, _, _ in g)
    argv = ["0", "wide", "classify/", "LH_GENE_TXT", "wide.interval", "UCSC_GENE2ISOFORM", "wide.map", "0", "100"]
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "oracle", "_ref", "lib"))
    p = subprocess.run([os.path.join(REF, "bin", "classify")] + argv, cwd=OUT, env=env, capture_output=True)
    files = sorted(os.listdir(os.path.join(OUT, "classify")))
    # classify.json, not case.json: the count / solve golden suites take every directory that has a case.json
    with open(os.path.join(OUT, "classify.json"), "w") as f:
        json.dump({"name": "wide", "classify": {"argv": argv, "exit": p.returncode, "files": files}}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("classify exit %d, files %s" % (p.returncode, files))


if __name__ == "__main__":
    main()
