"""The psi table's definition (include/lesseq_hip.h, lsq_ps_*) restated in plain Python from the interval, map and
MRF texts themselves -- no parser and no lookup structure of the library is involved: every read's junction set is tried against
every form's informative set -- and the hand-built inputs the psi tests share."""
import random

from golden_inputs import interval_line, mrf_line
from junction_ref import chromosomes, mrf_reads, write_case  # noqa: F401  (the texts' fields; no definition)

LIM = 1 << 30
REPORT = ("reads", "blocks", "occurrences", "dropped_overhang", "no_chromosome", "informative_occurrences", "counted", "several_events")


# ----------------------------------------------------------------------------- the definition

def line_introns(chrom, exons):
    """{(chrom, end of the left interval, start of the right one)}: the gaps between the maximal intervals of the union of the exons
    with end > start; an intron with an end outside (-2^30, 2^30) matches nothing and is none"""
    merged = []
    for s, e in sorted((s, e) for s, e in exons if e > s):
        if merged and s <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], e)
        else:
            merged.append([s, e])
    return {(chrom, a[1], b[0]) for a, b in zip(merged, merged[1:]) if -LIM < a[1] and b[0] < LIM}


def events_of(interval_text, map_text):
    """[(event, [(form, D(form))])]: the events of the map in bytewise name order (the order of count's table), an event's forms
    in the order of its lines in the map; of two isoform lines of one name the later one is the name's.  D(form): the form's
    introns that are not introns of every form of the event"""
    by_name = {}
    for line in interval_text.split("\n"):
        t = line.split()
        if len(t) >= 8:
            n = int(t[5])
            starts = [int(x) for x in t[6].split(",") if x]
            ends = [int(x) for x in t[7].split(",") if x]
            by_name[t[0]] = line_introns(t[1], list(zip(starts, ends))[:n])
    groups = {}
    for ln in map_text.split("\n"):
        t = ln.split()
        if len(t) >= 2:
            groups.setdefault(t[0], []).append(t[1])
    out = []
    for event in sorted(groups, key=lambda n: n.encode()):
        sets = [by_name[f] for f in groups[event]]
        common = set.intersection(*sets)
        out.append((event, [(f, s - common) for f, s in zip(groups[event], sets)]))
    return out


def read_junctions(blocks, known, min_overhang, rep):
    """S(r) of a read [(chrom, strand, start0, end)]: junctions' rule on neighbouring blocks in file order; the pairs that make no
    junction go to the report"""
    def chrom_of(b):
        c, _, s, e = b
        return c if c in known and -LIM < s < LIM and -LIM < e < LIM else None
    for a, b in zip(blocks, blocks[1:]):
        ca, cb = chrom_of(a), chrom_of(b)
        if ca is None or cb is None:
            rep["no_chromosome"] += 1
        elif ca == cb and b[2] > a[3]:
            if min(a[3] - a[2], b[3] - b[2]) < min_overhang:
                rep["dropped_overhang"] += 1
            else:
                rep["occurrences"] += 1
                yield (ca, a[3], b[2])


def table(interval_text, map_text, mrf_text, min_overhang=1):
    """(rows [(event, total, form, reads)] in table order, report, introns [|D(form)|] a row)"""
    known = set(chromosomes(interval_text))
    events = events_of(interval_text, map_text)
    informative = set().union(*[d for _, forms in events for _, d in forms]) if events else set()
    reads = mrf_reads(mrf_text)
    n_form = [[0] * len(forms) for _, forms in events]
    total = [0] * len(events)
    rep = dict.fromkeys(REPORT, 0)
    rep["reads"] = len(reads)
    for read in reads:
        rep["blocks"] += len(read)
        occ = list(read_junctions(read, known, min_overhang, rep))
        rep["informative_occurrences"] += sum(j in informative for j in occ)
        S = set(occ)
        n_events = 0
        for e, (_, forms) in enumerate(events):
            hit = [bool(S & d) for _, d in forms]
            for k, h in enumerate(hit):
                n_form[e][k] += h
            if any(hit):
                total[e] += 1
                n_events += 1
        rep["counted"] += n_events > 0
        rep["several_events"] += n_events > 1
    rows = [(event, total[e], f, n_form[e][k]) for e, (event, forms) in enumerate(events) for k, (f, _) in enumerate(forms)]
    return rows, rep, [len(d) for _, forms in events for _, d in forms]


def psi_of(rows, introns):
    """a row's psi, None for NA: x_f = reads_f / introns_f; den the sum of x_g over the event's forms in row order; x_f / den.  NA
    for every form of an event when one of its forms has introns 0 or den is 0"""
    out, i = [], 0
    while i < len(rows):
        j = i
        while j < len(rows) and rows[j][0] == rows[i][0]:
            j += 1
        if all(introns[k] > 0 for k in range(i, j)):
            x = [rows[k][3] / introns[k] for k in range(i, j)]
            den = 0.0
            for v in x:
                den += v
            out += [None] * (j - i) if den == 0 else [v / den for v in x]
        else:
            out += [None] * (j - i)
        i = j
    return out


def text(rows, introns=None):
    """the table; with `introns` the six columns of --psi"""
    if introns is None:
        return "".join("%s\t%d\t%s\t%d\n" % r for r in rows)
    return "".join("%s\t%d\t%s\t%d\t%d\t%s\n" % (r + (n, "NA" if p is None else "%.6f" % p)) for r, n, p in zip(rows, introns, psi_of(rows, introns)))


def map_of(isoform_lines):
    """the map text write_case writes"""
    return "".join("%s\t%s\n" % (ln.split("\t")[0].split(".")[0], ln.split("\t")[0]) for ln in isoform_lines)


def report_line(rep, n_introns, n_forms, n_events):
    """what the executable logs"""
    return ("psi: %d read(s), %d block(s), %d junction occurrence(s), %d block pair(s) below the overhang, %d with a block on no chromosome of the annotation; "
            "%d informative intron(s) of %d form(s) in %d event(s): %d occurrence(s) on them, %d read(s) counted, %d for more than one event"
            % (rep["reads"], rep["blocks"], rep["occurrences"], rep["dropped_overhang"], rep["no_chromosome"], n_introns, n_forms, n_events,
               rep["informative_occurrences"], rep["counted"], rep["several_events"]))


# ----------------------------------------------------------------------------- inputs

SE = [(1000, 1100), (1200, 1300), (1500, 1600)]


def definition_annotation():
    """an intron all forms share; three forms of which two share an informative intron; a skipped exon; one intron informative in
    two overlapping events; a one-form event; single-exon forms; a form whose exons overlap; the skipped exon again on another
    chromosome; an intron across the coordinate range's end"""
    I = interval_line
    return [I("A.1", "chr1", "+", [(100, 200), (300, 400), (500, 600), (700, 800)]),       # introns 200-300, 400-500, 600-700
            I("A.2", "chr1", "+", [(100, 200), (300, 400), (500, 800)]),                   # 200-300, 400-500
            I("A.3", "chr1", "+", [(100, 200), (300, 800)]),                               # 200-300: the one all three hold
            I("SE.inc", "chr1", "+", SE),
            I("SE.skp", "chr1", "+", [SE[0], SE[2]]),
            I("OV1.a", "chr1", "+", [(2000, 2100), (2200, 2300)]),                         # 2100-2200 ...
            I("OV1.b", "chr1", "+", [(2000, 2300)]),
            I("OV2.a", "chr1", "-", [(2050, 2100), (2200, 2400)]),                         # ... and again, in another event
            I("OV2.b", "chr1", "-", [(2050, 2100), (2250, 2400)]),
            I("ONE.a", "chr1", "+", [(3000, 3100), (3200, 3300)]),
            I("SG.a", "chr1", "+", [(4000, 4100)]),
            I("SG.b", "chr1", "+", [(4000, 4200)]),
            I("UN.a", "chr1", "+", [(5300, 5400), (5000, 5100), (5050, 5200)]),            # unsorted, overlapping: the union's gap is 5200-5300
            I("UN.b", "chr1", "+", [(5000, 5100), (5300, 5400), (5350, 5350)]),            # 5100-5300; an empty exon
            I("C2.inc", "chr2", "+", SE),
            I("C2.skp", "chr2", "+", [SE[0], SE[2]]),
            I("EDGE.a", "chr1", "+", [(LIM - 300, LIM - 200), (LIM - 150, LIM - 100), (LIM + 50, LIM + 100)]),      # the second intron matches nothing
            I("EDGE.b", "chr1", "+", [(LIM - 300, LIM - 100)])]


def definition_lines():
    m = mrf_line
    return [m("chr1", "+", [(150, 200), (300, 350)]),                                      # the intron all forms of A hold: nothing
            m("chr1", "+", [(350, 400), (500, 550)]),                                      # A.1 and A.2, A once
            m("chr1", "-", [(350, 400), (500, 600), (700, 750)]),                          # two informative introns of A.1: A.1 once
            m("chr1", "+", [(1050, 1100), (1200, 1300), (1500, 1550)]),                    # both inclusion junctions: SE.inc once
            m("chr1", "+", [(1050, 1100), (1500, 1550)]),                                  # SE.skp
            m("chr1", "+", [(1050, 1100), (1500, 1550), (1250, 1300), (1500, 1520)]),      # junctions of both forms: each once, SE once
            m("chr1", "+", [(2050, 2100), (2200, 2250)]),                                  # OV1.a and OV2.a: two events
            m("chr1", "+", [(2050, 2100), (2250, 2300)]),                                  # OV2.b
            m("chr1", "+", [(3050, 3100), (3200, 3250)]),                                  # the one form's intron: nothing
            m("chr1", "+", [(4000, 4100)]),
            m("chr1", "+", [(5150, 5200), (5300, 5350)]),                                  # UN.a
            m("chr1", "+", [(5050, 5100), (5300, 5350)]),                                  # UN.b
            m("chr1", "+", [(5050, 5100), (5200, 5250)]),                                  # an exon's end inside the union: no intron
            m("chr2", "+", [(1050, 1100), (1200, 1300), (1500, 1550)]),                    # C2.inc, not SE.inc
            m("chr1", "+", [(LIM - 250, LIM - 200), (LIM - 150, LIM - 120)]),              # EDGE.a
            m("chrU", "+", [(1050, 1100), (1500, 1550)])]                                  # a chromosome the annotation does not name


# what the definition gives on them, worked out by hand
DEFINITION_ROWS = [("A", 2, "A.1", 2), ("A", 2, "A.2", 2), ("A", 2, "A.3", 0), ("C2", 1, "C2.inc", 1), ("C2", 1, "C2.skp", 0), ("EDGE", 1, "EDGE.a", 1), ("EDGE", 1, "EDGE.b", 0),
                   ("ONE", 0, "ONE.a", 0), ("OV1", 1, "OV1.a", 1), ("OV1", 1, "OV1.b", 0), ("OV2", 2, "OV2.a", 1), ("OV2", 2, "OV2.b", 1),
                   ("SE", 3, "SE.inc", 2), ("SE", 3, "SE.skp", 2), ("SG", 0, "SG.a", 0), ("SG", 0, "SG.b", 0), ("UN", 2, "UN.a", 1), ("UN", 2, "UN.b", 1)]
DEFINITION_INTRONS = [2, 1, 0, 2, 1, 1, 0, 0, 1, 0, 1, 1, 2, 1, 0, 0, 1, 1]
DEFINITION_PSI = ["NA", "NA", "NA", "1.000000", "0.000000", "NA", "NA", "NA", "NA", "NA", "0.500000", "0.500000", "0.333333", "0.666667", "NA", "NA", "0.500000", "0.500000"]
DEFINITION_REPORT = {"reads": 16, "blocks": 36, "occurrences": 18, "dropped_overhang": 0, "no_chromosome": 1, "informative_occurrences": 15, "counted": 11, "several_events": 1}


def rule_lines(n=10):
    """the junction rule's edges around --min-overhang n, on the skipped exon's junctions: [(line, whether its skipping junction counts)]"""
    m = mrf_line
    a, b = SE[0][1], SE[2][0]
    big = [(200000 + 300 * k, 200000 + 300 * k + 100) for k in range(15)]
    return [(m("chr1", "+", [(a - n + 1, a), (b, b + 50)]), False),                        # overhang n - 1, left ...
            (m("chr1", "+", [(a - 50, a), (b, b + n - 1)]), False),                        # ... and right
            (m("chr1", "+", [(a - n, a), (b, b + 50)]), True),                             # n
            (m("chr1", "+", [(a - 50, a), (b, b + n)]), True),
            (m("chr1", "+", [(a - n - 1, a), (b, b + n + 1)]), True),                      # n + 1
            (m("chr1", "+", [(a - 50, a), (a, a + 50)]), False),                           # abutting
            (m("chr1", "+", [(a - 50, a), (a - 10, a + 50)]), False),                      # overlapping
            (m("chr1", "+", [(b, b + 50), (a - 50, a)]), False),                           # out of order
            (m("chr1", "+", [(a - 50, a)]).rstrip("\n") + "," + m("chr2", "+", [(b, b + 50)]), False),        # across two chromosomes
            (m("chr1", "+", [(a - 50, a)]).rstrip("\n") + "," + m("chrU", "+", [(b, b + 50)]), False),        # a block on no chromosome
            (m("chr1", "+", [(a - 50, a), (b, b + 50), (b + 60, b + 60)]), True),          # an empty block behind the junction
            (m("chr1", "+", [(a - 50, a)] + big), False),                                  # 16 blocks, none of the junctions an intron
            (m("chr1", "+", big + [(210000, 210050)]), False),
            (m("chr1", "+", [(900 - 100 * k, 950 - 100 * k) for k in range(14)][::-1] + [(a - 50, a), (b, b + 50)]), True)]      # ... the last of 16 blocks' 15 pairs


def random_case(seed=41, n_events=40, n_reads=5000):
    """(isoform lines, read tuples [(chrom, minus, blocks)]): about 40 events of two or three forms on three chromosomes -- chains
    of exons with some left out, a few forms of one exon, every fifth event a second set of forms over its predecessor's exons --
    and reads cut from the forms' exon chains (one to four ascending blocks, what a CIGAR can say), some beside every exon
    boundary, a few on an unnamed chromosome"""
    rng = random.Random(seed)
    iso, forms = [], []
    exons, chrom = None, None
    for g in range(n_events):
        if g % 5 != 4 or exons is None:
            chrom = "chr%d" % (1 + g % 3)
            x, exons = 1000 + 2500 * g + rng.randrange(200), []
            for _ in range(rng.randrange(3, 8)):
                w = rng.randrange(40, 150)
                exons.append((x, x + w))
                x += w + rng.randrange(60, 200)
        for j in range(rng.randrange(2, 4)):
            if rng.random() < 0.08:
                ex = [(exons[0][0], exons[-1][1])]
            else:
                ex = [e for k, e in enumerate(exons) if k in (0, len(exons) - 1) or rng.random() < 0.6]
            iso.append(interval_line("e%02d.%d" % (g, j), chrom, "+-"[g & 1], ex))
            forms.append((chrom, ex))
    reads = []
    for _ in range(n_reads):
        chrom, ex = forms[rng.randrange(len(forms))]
        if rng.random() < 0.03:
            chrom = "chrU"
        i = rng.randrange(len(ex))
        n = min(rng.choice((1, 2, 2, 2, 3, 4)), len(ex) - i)
        blocks = list(ex[i:i + n])
        if rng.random() < 0.85:
            if n > 1:
                blocks[0] = (max(blocks[0][0], blocks[0][1] - rng.randrange(1, 60)), blocks[0][1])
                blocks[-1] = (blocks[-1][0], min(blocks[-1][1], blocks[-1][0] + rng.randrange(1, 60)))
        else:           # beside the boundaries
            blocks = [(s + rng.choice((0, 0, 1)), e - rng.choice((0, 1, 2))) for s, e in blocks]
        reads.append((chrom, rng.random() < 0.5, blocks))
    return iso, reads


def count_case(n, seed=3):
    """(isoform lines, mrf lines): the definition annotation under n reads drawn from its own reads and a few more"""
    rng = random.Random(seed)
    pool = definition_lines() + [ln for ln, _ in rule_lines()]
    return definition_annotation(), [pool[rng.randrange(len(pool))] for _ in range(n)]


def deep_case(n_reads=1100):
    """(isoform lines, mrf lines): an event whose long form has 16 exons, reads of 1 to 16 of them in turn: the lanes of one wave
    hold between 0 and 15 pairs"""
    chain = [(1000 + 300 * k, 1100 + 300 * k) for k in range(16)]
    iso = [interval_line("D.long", "chr1", "+", chain), interval_line("D.odd", "chr1", "+", chain[::2]), interval_line("D.ends", "chr1", "+", [chain[0], chain[-1]]),
           interval_line("E.a", "chr1", "+", chain[3:9]), interval_line("E.b", "chr1", "+", [chain[3], chain[8]])]
    return iso, [mrf_line("chr1", "+", chain[k % 5:k % 5 + 1 + (k * 7) % 16][:16 - k % 5]) for k in range(n_reads)]


def hot_case(shuffled, n_hot=200000, n_rest=1000, seed=23):
    """(isoform lines, mrf lines): n_hot reads on one junction beside n_rest over the other events' junctions, in coordinate order
    or shuffled"""
    iso = []
    for g in range(6):
        b = 10000 * g
        iso += [interval_line("h%d.inc" % g, "chr1", "+", [(b + 1000, b + 1100), (b + 1200, b + 1300), (b + 1500, b + 1600)]),
                interval_line("h%d.skp" % g, "chr1", "+", [(b + 1000, b + 1100), (b + 1500, b + 1600)])]
    rng = random.Random(seed)
    reads = [(21100 - rng.randrange(1, 50), 21100, 21500, 21500 + rng.randrange(1, 50)) for _ in range(n_hot)]
    for _ in range(n_rest):
        b = 10000 * rng.choice((0, 1, 3, 4, 5))
        a, c = rng.choice(((1100, 1200), (1300, 1500), (1100, 1500), (1100, 1400)))
        reads.append((b + a - rng.randrange(1, 50), b + a, b + c, b + c + rng.randrange(1, 50)))
    if shuffled:
        rng.shuffle(reads)
    else:
        reads.sort()
    return iso, ["chr1:+:%d:%d:1:%d,chr1:+:%d:%d:%d:%d\n" % (s0 + 1, e0, e0 - s0, s1 + 1, e1, e0 - s0 + 1, e0 - s0 + e1 - s1) for s0, e0, s1, e1 in reads]


def fast_table(interval_text, map_text, mrf_text, min_overhang=1):
    """table() for inputs of many events: a read's junctions looked up in a dictionary from informative intron to the forms that
    hold it, where table() tries every form; test_psi_host checks it against table()"""
    known = set(chromosomes(interval_text))
    events = events_of(interval_text, map_text)
    holders = {}
    for e, (_, forms) in enumerate(events):
        for k, (_, d) in enumerate(forms):
            for j in d:
                holders.setdefault(j, []).append((e, k))
    reads = mrf_reads(mrf_text)
    n_form = [[0] * len(forms) for _, forms in events]
    total = [0] * len(events)
    rep = dict.fromkeys(REPORT, 0)
    rep["reads"] = len(reads)
    for read in reads:
        rep["blocks"] += len(read)
        occ = list(read_junctions(read, known, min_overhang, rep))
        rep["informative_occurrences"] += sum(j in holders for j in occ)
        hit = {ek for j in set(occ) for ek in holders.get(j, ())}
        for e, k in hit:
            n_form[e][k] += 1
        hit_events = {e for e, _ in hit}
        for e in hit_events:
            total[e] += 1
        rep["counted"] += len(hit_events) > 0
        rep["several_events"] += len(hit_events) > 1
    rows = [(event, total[e], f, n_form[e][k]) for e, (event, forms) in enumerate(events) for k, (f, _) in enumerate(forms)]
    return rows, rep, [len(d) for _, forms in events for _, d in forms]


def many_case(n_events=3000, seed=29):
    """(isoform lines, mrf lines): more forms, and more events, than a workgroup of the count kernel keeps counters of its own for:
    skipped-exon events 1000 bases apart, two reads on every event's skipping junction and one inclusion read on every seventh, shuffled"""
    iso = []
    for g in range(n_events):
        b = 1000 * g
        iso += [interval_line("m%04d.inc" % g, "chr1", "+", [(b, b + 100), (b + 200, b + 300), (b + 500, b + 600)]),
                interval_line("m%04d.skp" % g, "chr1", "+", [(b, b + 100), (b + 500, b + 600)])]
    rng = random.Random(seed)
    at = [(g, q) for g in range(n_events) for q in ((0, 0, 1) if g % 7 == 0 else (0, 0))]
    rng.shuffle(at)
    return iso, [mrf_line("chr1", "+", [(1000 * g + 50, 1000 * g + 100), (1000 * g + 200, 1000 * g + 300), (1000 * g + 500, 1000 * g + 540)] if q else
                          [(1000 * g + 60, 1000 * g + 100), (1000 * g + 500, 1000 * g + 530)]) for g, q in at]
