"""The evidence table's definition (include/lesseq_hip.h, lsq_fe_*) restated in plain Python from the interval, map
and MRF texts themselves -- no parser and no lookup structure of the library is involved: every read's junction set and every
block is tried against every form's informative introns and regions, and positions(f) is counted by laying a read at every start --
and the hand-built inputs the evidence tests share.  Events, forms, informative introns and a read's junctions are psi's
(tests/psi_ref.py), to the letter."""
import random

import psi_ref as V
from golden_inputs import interval_line, mrf_line
from junction_ref import chromosomes, mrf_reads, write_case  # noqa: F401  (the texts' fields; no definition)

LIM = V.LIM
REPORT = ("reads", "blocks", "occurrences", "dropped_overhang", "no_chromosome", "informative_occurrences", "skipped_blocks", "body_hits", "counted", "several_events",
          "counted_by_body_alone")


# ----------------------------------------------------------------------------- the definition

def union_of(exons):
    """U: the maximal intervals of the union of the exons with end > start"""
    merged = []
    for s, e in sorted((s, e) for s, e in exons if e > s):
        if merged and s <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], e)
        else:
            merged.append([s, e])
    return [tuple(m) for m in merged]


def minus(u, c):
    """u \\ c as maximal intervals, both lists of disjoint intervals ascending"""
    out = []
    for s, e in u:
        at = s
        for a, z in c:
            if z <= at or a >= e:
                continue
            if a > at:
                out.append((at, a))
            at = max(at, z)
        if at < e:
            out.append((at, e))
    return out


def both(u, v):
    return [(max(a, s), min(z, e)) for a, z in u for s, e in v if max(a, s) < min(z, e)]


def events_of(interval_text, map_text):
    """[(event, [(form, chrom, U(form), D(form), regions of B(form))])] in psi's order; regions clamped to [-2^30, 2^30], the empty ones dropped"""
    lines = {}
    for line in interval_text.split("\n"):
        t = line.split()
        if len(t) >= 8:
            n = int(t[5])
            starts = [int(x) for x in t[6].split(",") if x]
            ends = [int(x) for x in t[7].split(",") if x]
            lines[t[0]] = (t[1], union_of(list(zip(starts, ends))[:n]))
    out = []
    for event, forms in V.events_of(interval_text, map_text):
        common = None
        for f, _ in forms:
            chrom, u = lines[f]
            common = [(chrom, u)] if common is None else [(c, both(x, u)) for c, x in common if c == chrom]
        common = common[0][1] if common else []
        rows = []
        for f, d in forms:
            chrom, u = lines[f]
            regions = [(max(-LIM, a), min(LIM, z)) for a, z in minus(u, common)]
            rows.append((f, chrom, u, d, [(a, z) for a, z in regions if a < z]))
        out.append((event, rows))
    return out


def block_ok(b, known):
    c, _, s, e = b
    return c in known and s < e and -LIM < s < LIM and -LIM < e < LIM


def body_couples(blocks, known, chrom, regions, min_body):
    """the (block, region) couples of one form that pass the rule"""
    return sum(1 for b in blocks if block_ok(b, known) and b[0] == chrom for a, z in regions if min(b[3], z) - max(b[2], a) >= min_body)


def counts_for(blocks, known, min_overhang, min_body, chrom, d, regions):
    """whether the read counts for a form: a junction in D(f) or a block on a region of f"""
    rep = dict.fromkeys(V.REPORT, 0)
    return bool(set(V.read_junctions(blocks, known, min_overhang, rep)) & d) or body_couples(blocks, known, chrom, regions, min_body) > 0


def table(interval_text, map_text, mrf_text, min_overhang=1, min_body=1):
    """(rows [(event, total, form, reads)] in table order, report, introns [|D(form)|] a row, body [bases of B(form)] a row)"""
    known = set(chromosomes(interval_text))
    events = events_of(interval_text, map_text)
    informative = set().union(*[d for _, forms in events for _, _, _, d, _ in forms]) if events else set()
    reads = mrf_reads(mrf_text)
    n_form = [[0] * len(forms) for _, forms in events]
    total = [0] * len(events)
    rep = dict.fromkeys(REPORT, 0)
    rep["reads"] = len(reads)
    for read in reads:
        rep["blocks"] += len(read)
        rep["skipped_blocks"] += sum(not block_ok(b, known) for b in read)
        occ = list(V.read_junctions(read, known, min_overhang, rep))
        found = sum(j in informative for j in occ)
        rep["informative_occurrences"] += found
        S = set(occ)
        n_events = 0
        for e, (_, forms) in enumerate(events):
            any_form = False
            for k, (_, chrom, _, d, regions) in enumerate(forms):
                couples = body_couples(read, known, chrom, regions, min_body)
                rep["body_hits"] += couples
                if S & d or couples:
                    n_form[e][k] += 1
                    any_form = True
            total[e] += any_form
            n_events += any_form
        rep["counted"] += n_events > 0
        rep["several_events"] += n_events > 1
        rep["counted_by_body_alone"] += n_events > 0 and found == 0
    rows = [(event, total[e], f[0], n_form[e][k]) for e, (event, forms) in enumerate(events) for k, f in enumerate(forms)]
    return (rows, rep, [len(f[3]) for _, forms in events for f in forms], [sum(z - a for a, z in f[4]) for _, forms in events for f in forms])


def positions(interval_text, map_text, L, min_overhang=1, min_body=1):
    """a row's positions(f), by enumeration: every start of an ungapped L-base read along the form's concatenated exon union, its
    blocks the pieces of the union's intervals it covers, counted where the counting rule counts the read for f"""
    known = set(chromosomes(interval_text))
    out = []
    for _, forms in events_of(interval_text, map_text):
        for _, chrom, u, d, regions in forms:
            T = sum(e - s for s, e in u)
            n = 0
            for s in range(0, T - L + 1):
                blocks, off = [], 0
                for a, z in u:
                    lo, hi = max(s, off), min(s + L, off + z - a)
                    if lo < hi:
                        blocks.append((chrom, "+", a + lo - off, a + hi - off))
                    off += z - a
                n += counts_for(blocks, known, min_overhang, min_body, chrom, d, regions)
            out.append(n)
    return out


def psi_of(rows, pos):
    """a row's psi, None for NA: x_f = reads_f / positions_f; den the sum of x_g over the event's forms in row order; x_f / den.  NA
    for every form of an event when one of its forms has positions 0 or den is 0"""
    return V.psi_of(rows, pos)


def text(rows, introns=None, body=None, pos=None):
    """the table; with introns, body and positions the eight columns of --psi --read-length"""
    if introns is None:
        return "".join("%s\t%d\t%s\t%d\n" % r for r in rows)
    return "".join("%s\t%d\t%s\t%d\t%d\t%d\t%d\t%s\n" % (r + (n, b, q, "NA" if p is None else "%.6f" % p)) for r, n, b, q, p in zip(rows, introns, body, pos, psi_of(rows, pos)))


def report_line(rep, n_introns, n_regions, n_forms, n_events, min_overhang=1, min_body=1):
    """what the executable logs"""
    return ("evidence: %d read(s), %d block(s), %d junction occurrence(s), %d block pair(s) below the overhang, %d with a block on no chromosome of the annotation, "
            "%d block(s) skipped; %d informative intron(s) and %d body region(s) of %d form(s) in %d event(s): %d occurrence(s) and %d body hit(s) on them, "
            "%d read(s) counted, %d for more than one event, %d by body alone; min-overhang %d, min-body %d"
            % (rep["reads"], rep["blocks"], rep["occurrences"], rep["dropped_overhang"], rep["no_chromosome"], rep["skipped_blocks"], n_introns, n_regions, n_forms, n_events,
               rep["informative_occurrences"], rep["body_hits"], rep["counted"], rep["several_events"], rep["counted_by_body_alone"], min_overhang, min_body))


def fast_table(interval_text, map_text, mrf_text, min_overhang=1, min_body=1):
    """table() for inputs of many events or reads: a read's junctions looked up in a dictionary from informative intron to its
    forms, its blocks tried against the regions of a 4096-base window's list only; test_evidence_host checks it against table()"""
    known = set(chromosomes(interval_text))
    events = events_of(interval_text, map_text)
    holders, windows = {}, {}
    for e, (_, forms) in enumerate(events):
        for k, (_, chrom, _, d, regions) in enumerate(forms):
            for j in d:
                holders.setdefault(j, []).append((e, k))
            for a, z in regions:
                for w in range(a >> 12, ((z - 1) >> 12) + 1):
                    windows.setdefault((chrom, w), []).append((a, z, e, k))
    reads = mrf_reads(mrf_text)
    n_form = [[0] * len(forms) for _, forms in events]
    total = [0] * len(events)
    rep = dict.fromkeys(REPORT, 0)
    rep["reads"] = len(reads)
    for read in reads:
        rep["blocks"] += len(read)
        occ = list(V.read_junctions(read, known, min_overhang, rep))
        found = sum(j in holders for j in occ)
        rep["informative_occurrences"] += found
        hit = {ek for j in set(occ) for ek in holders.get(j, ())}
        for b in read:
            if not block_ok(b, known):
                rep["skipped_blocks"] += 1
                continue
            seen = set()
            for w in range(b[2] >> 12, ((b[3] - 1) >> 12) + 1):
                for item in windows.get((b[0], w), ()):
                    if item not in seen and min(b[3], item[1]) - max(b[2], item[0]) >= min_body:
                        seen.add(item)
            rep["body_hits"] += len(seen)
            hit |= {(e, k) for _, _, e, k in seen}
        for e, k in hit:
            n_form[e][k] += 1
        hit_events = {e for e, _ in hit}
        for e in hit_events:
            total[e] += 1
        rep["counted"] += len(hit_events) > 0
        rep["several_events"] += len(hit_events) > 1
        rep["counted_by_body_alone"] += len(hit_events) > 0 and found == 0
    rows = [(event, total[e], f[0], n_form[e][k]) for e, (event, forms) in enumerate(events) for k, f in enumerate(forms)]
    return (rows, rep, [len(f[3]) for _, forms in events for f in forms], [sum(z - a for a, z in f[4]) for _, forms in events for f in forms])


# ----------------------------------------------------------------------------- inputs

def definition_annotation():
    """psi's definition annotation and three events more: one interval that is a region in two events (OW1, OW2), and a region that
    reaches the coordinate range's end (EZ, on chr2).  The regions (worked out by hand):
    A.1 none (the common bases of A are its union); A.2 [600,700); A.3 [400,500) [600,700);  SE.inc [1200,1300);  OV1.b [2100,2200);
    OV2.a [2200,2250);  SG.b [4100,4200);  UN.a [5100,5200);  C2.inc chr2 [1200,1300);  EDGE.a none ([2^30+50, 2^30+100) is empty after
    clamping);  EDGE.b [2^30-200, 2^30-150);  OW1.a and OW2.a [6100,6300);  EZ.b chr2 [2^30-400, 2^30+100), clamped to [2^30-400, 2^30);
    none for SE.skp, OV1.a, OV2.b, ONE.a, SG.a, UN.b, C2.skp, OW1.b, OW2.b, EZ.a"""
    I = interval_line
    return V.definition_annotation() + [I("OW1.a", "chr1", "+", [(6000, 6400)]), I("OW1.b", "chr1", "+", [(6000, 6100), (6300, 6400)]),
                                        I("OW2.a", "chr1", "-", [(6050, 6350)]), I("OW2.b", "chr1", "-", [(6050, 6100), (6300, 6350)]),
                                        I("EZ.a", "chr2", "+", [(LIM - 500, LIM - 400)]), I("EZ.b", "chr2", "+", [(LIM - 500, LIM + 100)])]


def definition_lines():
    """psi's definition reads and reads for the body rule"""
    m = mrf_line
    return V.definition_lines() + [
        m("chr1", "+", [(1150, 1200)]),                                        # abuts SE.inc's region: nothing
        m("chr1", "+", [(1300, 1350)]),                                        # ... on the right
        m("chr1", "+", [(1150, 1350)]),                                        # contains the whole region: SE.inc
        m("chr1", "-", [(1199, 1201)]),                                        # one base of it, minus strand: SE.inc
        m("chr1", "+", [(450, 850)]),                                          # one block over both regions of A.3 (once) and A.2's: A once, three couples
        m("chr1", "+", [(610, 620), (630, 640)]),                              # two blocks in the region A.2 and A.3 share: each once, four couples
        m("chr1", "+", [(420, 440)]),                                          # the region A.3 alone has
        m("chr1", "+", [(1050, 1100), (1200, 1300), (1500, 1550)]),            # junctions and body of SE.inc: once
        m("chr1", "+", [(1220, 1260), (2050, 2100), (2250, 2300)]),            # body of SE.inc and the junction of OV2.b: two events
        m("chr1", "+", [(2120, 2180)]),                                        # OV1.b's region: a read through OV1.a's intron
        m("chr1", "-", [(2210, 2240)]),                                        # OV2.a's region, inside OV1's common exon
        m("chr1", "+", [(3120, 3180)]),                                        # the one-form event: nothing
        m("chr1", "+", [(4120, 4180)]),                                        # SG.b, the long form
        m("chr1", "+", [(4020, 4080)]),                                        # common bases of SG: nothing
        m("chr1", "+", [(1250, 1250)]),                                        # an empty block in a region: skipped
        m("chrU", "+", [(1220, 1260)]),                                        # no chromosome: skipped
        m("chr2", "+", [(1220, 1260)]),                                        # C2.inc, not SE.inc
        m("chr1", "+", [(LIM - 180, LIM - 160)]),                              # EDGE.b
        m("chr1", "+", [(LIM - 151, LIM - 120)]),                              # one base of EDGE.b's region, at its end
        m("chr1", "+", [(5120, 5180), (5300, 5350)]),                          # UN.a's region; 5180-5300 is a junction and no intron
        m("chr1", "+", [(6150, 6250)]),                                        # the region OW1.a and OW2.a share: two events
        m("chr1", "+", [(6050, 6100), (6300, 6350)]),                          # the intron OW1.b and OW2.b share: two events, no body (the blocks abut it)
        m("chr2", "+", [(LIM - 50, LIM - 1)]),                                 # EZ.b, up to the last coordinate a block can have
        m("chr2", "+", [(LIM - 350, LIM - 320)]),                              # EZ.b
        m("chr2", "+", [(LIM - 50, LIM)]),                                     # a block that ends outside the range: skipped
        m("chr1", "+", [(2190, 2260)])]                                        # 10 bases of OV1.b's region and the whole of OV2.a's 50: two events


# what the definition gives on them at the defaults, worked out by hand
DEFINITION_INTRONS = [2, 1, 0, 2, 1, 1, 0, 0, 0, 0, 1, 0, 1, 1, 0, 1, 0, 1, 2, 1, 0, 0, 1, 1]
DEFINITION_BODY = [0, 100, 200, 100, 0, 0, 50, 0, 400, 0, 0, 100, 50, 0, 200, 0, 200, 0, 100, 0, 0, 100, 100, 0]
DEFINITION_ROWS = [("A", 5, "A.1", 2), ("A", 5, "A.2", 4), ("A", 5, "A.3", 3), ("C2", 2, "C2.inc", 2), ("C2", 2, "C2.skp", 0), ("EDGE", 3, "EDGE.a", 1), ("EDGE", 3, "EDGE.b", 2),
                   ("EZ", 2, "EZ.a", 0), ("EZ", 2, "EZ.b", 2), ("ONE", 0, "ONE.a", 0), ("OV1", 3, "OV1.a", 1), ("OV1", 3, "OV1.b", 2), ("OV2", 5, "OV2.a", 3), ("OV2", 5, "OV2.b", 2),
                   ("OW1", 2, "OW1.a", 1), ("OW1", 2, "OW1.b", 1), ("OW2", 2, "OW2.a", 1), ("OW2", 2, "OW2.b", 1),
                   ("SE", 7, "SE.inc", 6), ("SE", 7, "SE.skp", 2), ("SG", 1, "SG.a", 0), ("SG", 1, "SG.b", 1), ("UN", 3, "UN.a", 2), ("UN", 3, "UN.b", 1)]
DEFINITION_REPORT = {"reads": 42, "blocks": 69, "occurrences": 25, "dropped_overhang": 0, "no_chromosome": 1, "informative_occurrences": 19, "skipped_blocks": 5,
                     "body_hits": 30, "counted": 30, "several_events": 5, "counted_by_body_alone": 16}


def edge_lines(n):
    """the body rule's edges around --min-body n on SE.inc's region [1200, 1300): [(line, whether it counts for SE.inc at min_body n)]"""
    m = mrf_line
    a, z = 1200, 1300
    return [(m("chr1", "+", [(a - 30, a + n - 1)]), False),                    # n - 1 bases at the left edge
            (m("chr1", "+", [(a - 30, a + n)]), True),                         # n
            (m("chr1", "+", [(a - 30, a + n + 1)]), True),                     # n + 1
            (m("chr1", "+", [(z - n + 1, z + 30)]), False),                    # ... at the right edge
            (m("chr1", "+", [(z - n, z + 30)]), True),
            (m("chr1", "-", [(z - n - 1, z + 30)]), True),
            (m("chr1", "+", [(a - 30, a)]), False),                            # abutting
            (m("chr1", "+", [(z, z + 30)]), False),
            (m("chr1", "+", [(a + 40, a + 40 + n)]), True),                    # n bases inside
            (m("chr1", "+", [(a + 40, a + 39 + n)]), False),                   # n - 1 inside (at n = 1 the block is empty)
            (m("chr1", "+", [(a - 30, z + 30)]), n <= 100),                    # the whole region
            (m("chr1", "+", [(a - 30, a + n - 1), (z - n + 1, z + 30)]), False)]      # two blocks of n - 1 each do not add up


def count_case(n, seed=3):
    """(isoform lines, mrf lines): the definition annotation under n reads drawn from both tools' definition reads and the edges'"""
    rng = random.Random(seed)
    pool = definition_lines() + [ln for ln, _ in V.rule_lines()] + [ln for ln, _ in edge_lines(10)]
    return definition_annotation(), [pool[rng.randrange(len(pool))] for _ in range(n)]


def spread_case(n_events=40, n_reads=320):
    """(isoform lines, mrf lines): n_events retained-intron events 200 bases apart and, in every wave of 64 reads, one read whose one
    block covers all their retained introns; the wave's other lanes lie between events"""
    iso = []
    for g in range(n_events):
        b = 10000 + 200 * g
        iso += [interval_line("s%02d.ret" % g, "chr1", "+", [(b, b + 150)]), interval_line("s%02d.spl" % g, "chr1", "+", [(b, b + 50), (b + 100, b + 150)])]
    wide = mrf_line("chr1", "+", [(10000, 10000 + 200 * n_events)])
    quiet = mrf_line("chr1", "+", [(10160, 10190)])
    return iso, [wide if k % 64 == 17 else quiet for k in range(n_reads)]


def nested_case(n_small=500, seed=5):
    """(isoform lines, mrf lines): n_small skipped-exon events inside the retained intron of one long event; blocks inside the long
    region that overlap none, one or a few of the small ones"""
    iso = [interval_line("L.ret", "chr1", "+", [(1000, 1000 + 300 * n_small + 2000)]),
           interval_line("L.spl", "chr1", "+", [(1000, 1500), (1000 + 300 * n_small + 1500, 1000 + 300 * n_small + 2000)])]
    for g in range(n_small):
        b = 2000 + 300 * g
        iso += [interval_line("n%03d.inc" % g, "chr1", "-", [(b, b + 50), (b + 100, b + 150), (b + 200, b + 250)]),
                interval_line("n%03d.skp" % g, "chr1", "-", [(b, b + 50), (b + 200, b + 250)])]
    rng = random.Random(seed)
    lines = []
    for _ in range(700):
        s = 1600 + rng.randrange(300 * n_small)
        lines.append(mrf_line("chr1", "+", [(s, s + rng.choice((20, 60, 100, 400, 900)))]))
    return iso, lines


def hot_case(shuffled, n_hot=200000, n_rest=1000, seed=23):
    """(isoform lines, mrf lines): n_hot unspliced reads inside one retained intron beside n_rest over the other events, in
    coordinate order or shuffled"""
    iso = []
    for g in range(6):
        b = 10000 * g
        iso += [interval_line("h%d.ret" % g, "chr1", "+", [(b + 1000, b + 3000)]), interval_line("h%d.spl" % g, "chr1", "+", [(b + 1000, b + 1500), (b + 2500, b + 3000)])]
    rng = random.Random(seed)
    reads = []
    for _ in range(n_hot):
        s = 21500 + rng.randrange(0, 950)
        reads.append((s, s + 50))
    for _ in range(n_rest):
        b = 10000 * rng.choice((0, 1, 3, 4, 5))
        kind = rng.randrange(3)
        if kind == 0:
            s = b + 1500 + rng.randrange(0, 950)
            reads.append((s, s + 50))
        elif kind == 1:
            k = rng.randrange(1, 50)
            reads.append((b + 1500 - k, b + 1500, b + 2500, b + 2550 - k))
        else:
            s = b + 1000 + rng.randrange(0, 400)
            reads.append((s, s + 50))
    if shuffled:
        rng.shuffle(reads)
    else:
        reads.sort()
    return iso, [mrf_line("chr1", "+", [r[:2]] if len(r) == 2 else [r[:2], r[2:]]) for r in reads]


def many_case(n_events=3000, seed=29):
    """(isoform lines, mrf lines): more forms, and more events, than a workgroup of the count kernel keeps counters of its own for:
    psi's skipped-exon events, two skipping reads on every event, one read in the skipped exon's body on every seventh, shuffled"""
    iso, _ = V.many_case(n_events, seed)
    rng = random.Random(seed)
    at = [(g, q) for g in range(n_events) for q in ((0, 0, 1) if g % 7 == 0 else (0, 0))]
    rng.shuffle(at)
    return iso, [mrf_line("chr1", "+", [(1000 * g + 210, 1000 * g + 260)] if q else [(1000 * g + 60, 1000 * g + 100), (1000 * g + 500, 1000 * g + 530)]) for g, q in at]
