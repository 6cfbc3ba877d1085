#!/usr/bin/env python3
"""Capture tests/golden/gtf/: GTF inputs invented here from a seed, and what the reference's own prebuilt
bin/parseGencode and bin/gencodeIsoformMap print for them -- standard output, standard error and exit status, each
recorded.  CPU only, run in a build tree that has the reference next to it:

    python tools/make_gtf_golden.py              # writes tests/golden/gtf/
    python tools/make_gtf_golden.py --time       # times the reference on the GTF of tools/gtf_bench.py instead

Per case directory: in.gtf, out.interval (stdout), out.stderr, status (exit status), and for a case that parses names.txt
(`cut -f1 out.interval`) and out.map (gencodeIsoformMap on it).  mapnames/: <case>.names and <case>.map.
Nothing of the reference is copied: only what its programs read and wrote.  A case on which the reference ends with a
signal is refused, so a fixture can never record a crash as truth.

Case sets:
  cuff     Cufflinks-shaped: transcript + exon lines, FPKM attributes, both strands, several chromosomes, interleaved and
           non-contiguous transcripts, exons out of order, a duplicate exon, one transcript id under two genes,
           transcript_id ahead of gene_id
  gencode  GENCODE-shaped lines (gene, transcript, exon, CDS, UTR, start_codon; a dozen attributes, unquoted `level 2`,
           repeated tag, quoted values with blanks and semicolons), no '#' lines, ids that separate two-key order from
           joined-name order, upper and lower case, one 10 KB line, attribute oddities the reference accepts, "\\r\\n",
           no newline at the end
  numbers  atoi cases; nested and equal-start exons (the two lists sorted on their own); a transcript of a few hundred
           scattered lines on two chromosomes (the first kept line gives chromosome and strand)
  errors/  one file per "PROBLEM:" message, the bad line late in the file
  mapnames hand-made name lists for gencodeIsoformMap
"""
import os
import random
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "gtf")
REF = os.environ.get("LSQ_REFERENCE", "/root/reference")


def run_ref(tool, data):
    p = subprocess.run([os.path.join(REF, "bin", tool)], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if p.returncode < 0 or p.returncode >= 128:
        raise SystemExit("the reference's %s ended with status %d (a signal): this input cannot be a fixture" % (tool, p.returncode))
    return p.returncode, p.stdout, p.stderr


def line(chrom, feature, start, end, strand, attrs, source="src"):
    return "%s\t%s\t%s\t%s\t%s\t.\t%s\t.\t%s\n" % (chrom, source, feature, start, end, strand, attrs)


def cuff():
    rng = random.Random(20261016)
    tx = []         # (gene, transcript, chrom, strand, exons)
    for g in range(14):
        chrom = "chr%s" % rng.choice(["1", "2", "7", "X", "12"])
        strand = rng.choice("+-")
        base = 5000 + 30000 * g
        for t in range(rng.randint(1, 4)):
            exons, pos = [], base + rng.randrange(0, 300)
            for _ in range(rng.randint(1, 9)):
                ln = rng.randrange(40, 500)
                exons.append((pos, pos + ln))
                pos += ln + rng.randrange(80, 2000)
            tx.append(("CUFF.%d" % g, "CUFF.%d.%d" % (g, t + 1), chrom, strand, exons))
    tx.append(("CUFF.3", "SHARED.1", "chr2", "+", [(100, 200), (300, 400)]))       # one transcript id under two genes
    tx.append(("CUFF.9", "SHARED.1", "chr7", "-", [(700, 900)]))
    blocks = []
    for i, (g, t, chrom, strand, exons) in enumerate(tx):
        ex = list(exons)
        if i % 3 == 0:
            rng.shuffle(ex)                                   # exons out of order
        if i == 4:
            ex.append(ex[0])                                  # a duplicate exon
        fpkm = 'FPKM "%.10f"; frac "%.6f"; conf_lo "0.000000"; conf_hi "%.6f"; cov "%.6f";' % (rng.random() * 50, rng.random(), rng.random() * 90, rng.random() * 30)
        ids = 'gene_id "%s"; transcript_id "%s";' % (g, t) if i % 4 else 'transcript_id "%s"; gene_id "%s";' % (t, g)
        head = line(chrom, "transcript", min(s for s, _ in ex), max(e for _, e in ex), strand, ids + " " + fpkm, "Cufflinks")
        rows = [line(chrom, "exon", s, e, strand, '%s exon_number "%d"; %s' % (ids, k + 1, fpkm), "Cufflinks") for k, (s, e) in enumerate(ex)]
        blocks.append([head] + rows)
    # interleaved and non-contiguous: the rows of neighbouring transcripts are dealt out in turn, two transcripts are split in halves
    out = []
    for a in range(0, len(blocks), 3):
        grp = blocks[a:a + 3]
        if a % 2 == 0:
            while any(grp):
                for b in grp:
                    if b:
                        out.append(b.pop(0))
        else:
            for b in grp:
                out.extend(b)
    tail = out[5:9]
    del out[5:9]
    return "".join(out + tail).encode()


def gencode():
    rng = random.Random(7)
    genes = ["B", "G", "G-1", "G.1", "G10", "G2", "a", "ENSG00000223972.5", "ensg1"]      # two-key order differs from joined-name order
    rows = []
    for gi, g in enumerate(genes):
        chrom, strand, base = "chr%d" % (1 + gi % 3), "+-"[gi % 2], 11000 + 9000 * gi
        for tn in (["x"] if gi < 7 else ["ENST0000045%d.2" % k for k in range(3)]) + (["X"] if g == "G2" else []):
            common = ('gene_id "%s"; transcript_id "%s"; gene_type "transcribed_unprocessed_pseudogene"; gene_name "DDX11L%d"; transcript_type "processed_transcript"; '
                      'transcript_name "DDX11L%d-20%d";' % (g, tn, gi, gi, len(tn)))
            rows.append(line(chrom, "gene", base, base + 5000, strand, common + " level 2;", "HAVANA"))
            rows.append(line(chrom, "transcript", base, base + 5000, strand, common + ' level 2; tag "basic"; transcript_support_level "1";', "HAVANA"))
            pos = base
            for x in range(rng.randint(2, 6)):
                ln = rng.randrange(50, 300)
                attrs = common + ' exon_number %d; exon_id "ENSE0000%07d.1"; level 2; tag "basic"; tag "a b"; note "x;y"; havana_gene "OTTHUMG0000000096%d.2";' % (x + 1, rng.randrange(10 ** 6), gi)
                rows.append(line(chrom, "exon", pos, pos + ln, strand, attrs, "HAVANA"))
                if x % 2:
                    rows.append(line(chrom, "CDS", pos + 3, pos + ln - 3, strand, attrs + ' protein_id "ENSP%d";' % x, "HAVANA"))
                if x == 0:
                    rows.append(line(chrom, "UTR", pos, pos + 2, strand, attrs, "HAVANA"))
                    rows.append(line(chrom, "start_codon", pos + 3, pos + 5, strand, attrs, "HAVANA"))
                pos += ln + rng.randrange(100, 900)
    # features that are not `exon` exactly
    rows.append(line("chr1", "Exon", 1, 2, "+", 'gene_id "B"; transcript_id "x";'))
    rows.append(line("chr1", "exons", 1, 2, "+", 'gene_id "B"; transcript_id "x";'))
    # one 10 KB line: tags ahead of the ids
    rows.append(line("chr4", "exon", 500, 600, "+", " ".join('tag "filler_%04d";' % k for k in range(560)) + ' gene_id "LONG"; transcript_id "LONG.1";'))
    # attribute syntax the reference accepts
    rows.append(line("chr5", "exon", 10, 20, "-", 'gene_id "ODD"; transcript_id "nosemi"'))
    rows.append(line("chr5", "exon", 30, 40, "-", 'gene_id "ODD";transcript_id "noblank";'))
    rows.append(line("chr5", "exon", 50, 60, "-", 'gene_id  "ODD";  transcript_id   "twoblanks"  ;'))
    rows.append(line("chr5", "exon", 70, 80, "-", 'gene_id "ODD"; gene_id "SECOND"; transcript_id "firstwins";'))
    rows.append(line("chr5", "exon", 90, 95, "-", 'gene_id"ODD"; transcript_id "noblankbeforequote";'))
    rows.append(line("chr5", "exon", 96, 99, "-", 'xgene_id "SUB"; gene_id "ODD"; xtranscript_idy "substring"; transcript_id "T";'))
    rows.append(line("chr5", "exon", 100, 110, "-", 'note "my gene_id"; gene_id "ODD"; transcript_id "keyinvalue";'))
    rows.append(line("chr5", "exon", 120, 130, "-", 'gene_id "A" "B"; transcript_id "firsttolastquote";'))
    rows.append(line("chr5", "exon", 140, 150, "-", 'gene_id "ODD;cut"; transcript_id "onequote'))
    rows.append(line("chr5", "exon", 160, 170, "-", 'gene_id ""; transcript_id "emptygene";'))
    rows.append(line("chr5", "exon", 180, 190, "-", 'gene_id "G H"; transcript_id "T U"; level'))
    rows.append(line("chr5", "exon", 200, 210, "-", 'gene_id "ODD"; transcript_id "tenthfield";').rstrip("\n") + "\textra\tfields\n")
    rows.append(line("", "exon", 220, 230, "", 'gene_id "ODD"; transcript_id "emptychrom";'))
    rows.append(line("chr5", "exon", 240, 250, "-", 'gene_id "ODD"; transcript_id "crlf";').rstrip("\n") + "\r\n")
    rows.append(line("chr5", "exon", 260, 270, "-", 'gene_id "ODD"; transcript_id "crcrlf').rstrip("\n") + "\r\r\n")
    rows.append(line("chr5", "exon", 280, 290, "-", 'GENE_ID "CASE"; gene_id "ODD"; transcript_id "lastlinenonewline";').rstrip("\n"))
    return "".join(rows).encode()


# lines of the scattered transcript of `numbers` (the first-kept-line rule was also probed with 2 600: the same answer)
BIG_LINES = 500


def numbers():
    rng = random.Random(99)
    ids = 'gene_id "%s"; transcript_id "%s";'
    rows = []
    for k, (s, e) in enumerate([("", "7"), ("1.5", "9"), ("3000000000", "3000000001"), ("-5", "-2"), (" +12x", "0012"), ("99999999999999999999", "-99999999999999999999"),
                                ("-2147483648", "2147483648"), ("abc", "4e3"), ("2147483647", "2147483647"), ("0", "0"), ("\v\f7", "+-3")]):
        rows.append(line("chr1", "exon", s, e, "+", ids % ("ATOI", "atoi.%02d" % k)))
    for s, e in [(100, 500), (200, 300), (50, 600)]:
        rows.append(line("chr2", "exon", s, e, "+", ids % ("NEST", "nested")))
    for e in [900, 300, 700, 300, 100, 800, 150, 400]:
        rows.append(line("chr2", "exon", 100, e, "-", ids % ("NEST", "equalstart")))
    for chrom, strand in [("chr1", "+"), ("chr9", "-"), ("chr5", "-"), ("chr7", "+")]:
        rows.append(line(chrom, "exon", 10, 20, strand, ids % ("SPLIT", "fwd")))
    for chrom, strand in [("chr7", "+"), ("chr5", "-"), ("chr9", "-"), ("chr1", "+")]:
        rows.append(line(chrom, "exon", 10, 20, strand, ids % ("SPLIT", "rev")))
    # a few thousand scattered lines of one transcript, its first kept line on chr3 -, later ones (with smaller coordinates) on chr8 +
    big = [line("chr3", "exon", 500000, 500010, "-", ids % ("SPLIT", "big"))]
    for k in range(BIG_LINES):
        s = rng.randrange(1, 400000)
        big.append(line("chr8" if k % 2 else "chr3", "exon", s, s + rng.randrange(1, 50), "+" if k % 2 else "-", ids % ("SPLIT", "big")))
    other = [line("chr6", "exon", 100 + 10 * k, 105 + 10 * k, "+", ids % ("FILL%d" % (k % 40), "fill.%d" % (k % 80))) for k in range(120)]
    mixed = big[1:] + other
    rng.shuffle(mixed)
    return "".join(rows + big[:1] + mixed).encode()


def errors():
    good = "".join(line("chr1", "exon", 100 + 50 * k, 120 + 50 * k, "+", 'gene_id "OK"; transcript_id "ok.%d";' % (k % 5)) for k in range(60))
    bad = {
        "missing_gene_id": line("chr1", "exon", 1, 2, "+", 'transcript_id "T";'),
        "missing_transcript_id": line("chr1", "exon", 1, 2, "+", 'gene_id "G"; level 2;'),
        "missing_transcript_id_on_a_gene_line": line("chr1", "gene", 1, 2, "+", 'gene_id "G"; level 2;'),
        "unquoted_gene_id": line("chr1", "exon", 1, 2, "+", "gene_id A"),
        "unquoted_transcript_id": line("chr1", "exon", 1, 2, "+", 'gene_id "G"; transcript_id T; level 2;'),
        "unquoted_both": line("chr1", "CDS", 1, 2, "+", "transcript_id T; gene_id A;"),
        "two_bad_lines": line("chr1", "exon", 1, 2, "+", 'gene_id "G";') + good[:200] + line("chr1", "exon", 1, 2, "+", "gene_id A"),
    }
    return {k: (good + v + good[:300]).encode() for k, v in bad.items()}


MAPNAMES = {
    "returning_gene": b"G1|a\nG1|b\nG2|c\nG1|d\n",
    "several_bars": b"G|a|b\nG|c|d|e\nH||x\n|y\n|z\nH|\n",
    "tab_in_line": b"G|a\tchr1\t+\nG|b\tx\nK|c\t\n",
    "no_final_newline": b"G|a\nH|b",
    "empty_lines_and_cr": b"\nG|a\r\n\nG|b\r\r\n\r\nH|c\rx\n",
    "one_line_without_bar": b"abc\n",
    "empty": b"",
}


def write(path, data):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)


def capture_gtf(name, data):
    d = os.path.join(OUT, name)
    rc, out, err = run_ref("parseGencode", data)
    write(os.path.join(d, "in.gtf"), data)
    write(os.path.join(d, "out.interval"), out)
    write(os.path.join(d, "out.stderr"), err)
    write(os.path.join(d, "status"), b"%d\n" % rc)
    if rc == 0:
        names = b"".join(l.split(b"\t", 1)[0] + b"\n" for l in out.split(b"\n")[:-1])
        mrc, mout, merr = run_ref("gencodeIsoformMap", names)
        if mrc != 0 or merr:
            raise SystemExit("%s: gencodeIsoformMap exits %d on the names" % (name, mrc))
        write(os.path.join(d, "names.txt"), names)
        write(os.path.join(d, "out.map"), mout)
    print("%-48s status %d, %6d bytes in, %6d out" % (name, rc, len(data), len(out)))


def time_reference():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gtf_bench
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "bench.gtf")
        n_lines, n_exon = gtf_bench.generate(path)
        t0 = time.perf_counter()
        with open(path, "rb") as f, open(os.path.join(d, "bench.interval"), "wb") as o:
            rc = subprocess.run([os.path.join(REF, "bin", "parseGencode")], stdin=f, stdout=o).returncode
        t1 = time.perf_counter()
        with open(os.path.join(d, "bench.interval"), "rb") as f:
            names = subprocess.run(["cut", "-f1"], stdin=f, stdout=subprocess.PIPE).stdout
        t2 = time.perf_counter()
        mrc = subprocess.run([os.path.join(REF, "bin", "gencodeIsoformMap")], input=names, stdout=subprocess.DEVNULL).returncode
        t3 = time.perf_counter()
        print("%d lines (%d exon), %d bytes: parseGencode %.2f s (status %d), gencodeIsoformMap %.2f s (status %d)"
              % (n_lines, n_exon, os.path.getsize(path), t1 - t0, rc, t3 - t2, mrc))


def main():
    if not os.path.isdir(os.path.join(REF, "bin")):
        raise SystemExit("no reference tree at %s" % REF)
    if "--time" in sys.argv[1:]:
        return time_reference()
    shutil.rmtree(OUT, ignore_errors=True)
    capture_gtf("cuff", cuff())
    capture_gtf("gencode", gencode())
    capture_gtf("numbers", numbers())
    for k, v in errors().items():
        capture_gtf("errors/" + k, v)
    for k, v in MAPNAMES.items():
        rc, out, err = run_ref("gencodeIsoformMap", v)
        if rc != 0 or err:
            raise SystemExit("mapnames/%s: status %d" % (k, rc))
        write(os.path.join(OUT, "mapnames", k + ".names"), v)
        write(os.path.join(OUT, "mapnames", k + ".map"), out)
        print("%-48s status %d" % ("mapnames/" + k, rc))


if __name__ == "__main__":
    main()
