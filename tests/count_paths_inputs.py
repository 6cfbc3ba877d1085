"""Inputs of tests/test_count_cells_host.py and tests/test_count_paths_gpu.py: the hand-made events of the threshold test
(tests/test_parity_gpu.py), two more, seeded small gene sets, and the case files -- reads that the model (count_cells_ref.py)
picks for one verdict of one streaming kernel each.  Test infrastructure only."""
import bisect
import random

import count_cells_ref as cr
import golden_inputs as gi

CHROM = "chr1"
# event A (long form splits its first exon in two abutting segments): segments [1000,1100) [1100,1160) [1400,1500)
# event B (skipped exon):                                             segments [2000,2100) [2300,2360) [2600,2700)
# event C overlaps A's last segment and B's first (its own segments abut once): [1450,1520) [1520,1600) [2050,2130)
ABC = [("A", "+", [[(1000, 1160), (1400, 1500)], [(1000, 1100), (1400, 1500)]]),
       ("B", "+", [[(2000, 2100), (2300, 2360), (2600, 2700)], [(2000, 2100), (2600, 2700)]]),
       ("C", "-", [[(1450, 1600), (2050, 2130)], [(1450, 1520), (2050, 2130)]])]
ABC_SEGS = {"A": [(1000, 1100), (1100, 1160), (1400, 1500)], "B": [(2000, 2100), (2300, 2360), (2600, 2700)],
            "C": [(1450, 1520), (1520, 1600), (2050, 2130)]}
# event D lies where A's last segment and C's first overlap: the bases [1471,1490) are covered by three segments, and D's
#         first base by two others'; its last two segments abut and begin inside C's last, so that reads can run past the
#         end of C's last segment (which nothing abuts) and still be loaded:    [1470,1490) [2110,2160) [2160,2200)
# event E starts inside A's first segment (its first base is also inside another event's segment), runs over A's second and
#         on; its last two segments abut (a junction into an abutting run):    [1040,1180) [1200,1225) [1225,1250)
DE = [("D", "+", [[(1470, 1490), (2110, 2200)], [(1470, 1490), (2110, 2160)]]),
      ("E", "+", [[(1040, 1180), (1200, 1250)], [(1040, 1180), (1200, 1225)]])]
DE_SEGS = {"D": [(1470, 1490), (2110, 2160), (2160, 2200)], "E": [(1040, 1180), (1200, 1225), (1225, 1250)]}


def annotation_text(genes):
    """(interval text, map text) of genes given as (name, strand, [exon list of each isoform])"""
    iv = mp = ""
    for name, strand, forms in genes:
        for q, exons in enumerate(forms):
            iv += gi.interval_line("%s.%d" % (name, q), CHROM, strand, exons)
            mp += "%s\t%s.%d\n" % (name, name, q)
    return iv, mp


def write_annotation(d, stem, genes):
    iv, mp = annotation_text(genes)
    with open("%s/%s.interval" % (d, stem), "w") as f:
        f.write(iv)
    with open("%s/%s.map" % (d, stem), "w") as f:
        f.write(mp)
    return "%s/%s.interval" % (d, stem), "%s/%s.map" % (d, stem)


def seeded_genes(seed):
    """three to six genes of one to three isoforms on a coarse grid of coordinates, so that segments of different genes overlap,
    abut and share ends often: two- and three-owner stretches, first bases inside other genes' segments"""
    rng = random.Random(seed)
    genes = []
    for g in range(rng.randint(3, 6)):
        x = 1000 + 20 * rng.randint(0, 12)
        exons = []
        for _ in range(rng.randint(2, 3)):
            ln = 10 * rng.randint(1, 6)
            exons.append((x, x + ln))
            x += ln + 10 * rng.randint(1, 5)
        forms = [exons]
        if rng.random() < 0.8:          # a form that skips a middle or last exon
            k = rng.randrange(1, len(exons))
            forms.append(exons[:k] + exons[k + 1:])
        if rng.random() < 0.5:          # a form whose first exon ends early: two abutting segments
            s, e = exons[0]
            if e - s >= 20:
                forms.append([(s, e - 10)] + exons[1:])
        genes.append(("G%d" % g, "+-"[rng.randint(0, 1)], forms))
    return genes


def models_of(ev):
    """per packed bucket of compiled events: (bucket, Model of its events from the library's own segments, their output indices)"""
    out = []
    for b in range(ev.num_buckets):
        kind, idx = ev.bucket_events(b)
        if kind != 1:
            continue
        events = [cr.Event(ev.gene_name(i), ev.segments(i)) for i in idx]
        M = cr.Model(events)
        assert [e.name for e in M.events] == [e.name for e in events], "the bucket's order is (span start, span end, index)"
        out.append((b, M, idx))
    return out


def threshold_reads(with_strands=False):
    """the reads of test_reads_on_every_threshold_of_the_streaming_loops_vs_oracle (tests/test_parity_gpu.py, which takes them
    from here), as tuples (a, b) / (a, y, z, w) in file order; with_strands: (read, strand) pairs"""
    ends = sorted({1100, 1160, 1500, 1520, 1600, 2100, 2130, 2360, 2700})
    starts = sorted({1000, 1100, 1400, 1450, 1520, 2000, 2050, 2300, 2600})
    reads = []
    # one-block reads: every start region x every end -1 / 0 / +1 / +2 / +30, several lengths
    for s0 in (1001, 1040, 1099, 1101, 1130, 1401, 1449, 1451, 1470, 1499, 1501, 1530, 2001, 2049, 2051, 2080, 2099, 2101, 2120, 2301, 2601):
        for e in ends:
            for d in (-1, 0, 1, 2, 30):
                if e + d > s0 and e + d - s0 < 900:
                    reads.append(((s0, e + d), "+" if (s0 + e) % 3 else "-"))
    # two-block reads: block 1 ends on / beside every segment end, block 2 starts on / beside every later segment start or
    # touches block 1; block 2 lengths put 50 |block 1| against 49 total on and around equality
    for s0 in (1005, 1030, 1060, 1099, 1105, 1140, 1405, 1455, 1470, 1490, 1525, 1560, 2005, 2030, 2055, 2070, 2090, 2105, 2305, 2340):
        for e in ends:
            for d1 in (-1, 0, 1):
                y = e + d1
                if not (0 < y - s0 < 300):
                    continue
                l1 = y - s0
                for z0 in starts:
                    for dz in (0, 1):
                        z = z0 + dz
                        if z < y:
                            continue
                        for l2 in sorted({1, 2, max(1, l1 // 49), l1 // 49 + 1, 20, 60, 100, 131}):
                            reads.append(((s0, y, z, z + l2), "+" if (s0 + z + l2) % 5 else "-"))
                # touching blocks, listed in ascending order: the loader merges them into ONE block (interval_list::add_interval),
                # so these never reach the exception list; tests/test_count_paths_gpu.py lists such blocks the other way round
                reads.append(((s0, y, y, y + 7), "+"))
    return reads if with_strands else [r for r, _ in reads]


def covered_block(cov, a, b):
    """the block lies inside one covered region (Events.covered): the loader keeps it"""
    return any(s <= a and b <= e for s, e in cov)


def loadable(cov, rd):
    """every block of the read is kept"""
    return covered_block(cov, rd[0], rd[1]) and (len(rd) == 2 or covered_block(cov, rd[2], rd[3]))


def add_interval(S, E, s, e):
    """interval_list::add_interval as the reference has it (jsc/util/interval_list.hpp:462-503; csrc/lsq_annot.cpp IntervalList::add):
    the merge a read's blocks go through.  An interval that ends exactly where the new one starts is merged with it, one that
    starts exactly where the new one ends is not."""
    if not s < e:
        return
    ss, se, es, ee = bisect.bisect_left(S, s), bisect.bisect_left(E, s), bisect.bisect_left(S, e), bisect.bisect_left(E, e)
    start_inside, end_inside = ss - se == 1, es - ee == 1
    del S[ss:es]
    del E[se:ee]
    if not start_inside:
        S.insert(ss, s)
    if not end_inside:
        E.insert(se, e)


def file_blocks(rd, forward=False):
    """the blocks of a read in the order its line lists them: as given, but touching blocks (z == y) second block first unless
    `forward` -- listed in ascending order they would be merged into one block by the loader, listed so they stay two"""
    if len(rd) == 2:
        return [(rd[0], rd[1])]
    blocks = [(rd[0], rd[1]), (rd[2], rd[3])]
    return blocks[::-1] if rd[2] == rd[1] and not forward else blocks


def loaded(cov, rd, forward=False):
    """the read as the count kernel gets it: the blocks the loader keeps (each inside one covered region), merged in file
    order; None when no block is kept (or more than two come of it)"""
    S, E = [], []
    for a, b in file_blocks(rd, forward):
        if covered_block(cov, a, b):
            add_interval(S, E, a, b)
    if len(S) == 1:
        return (S[0], E[0])
    return (S[0], E[0], S[1], E[1]) if len(S) == 2 else None


def mrf_text(reads, forward=False, strands=None):
    """reads as (a, b) / (a, y, z, w); without `strands` the strand alternates (it plays no part off the span-start ties)"""
    return "AlignmentBlocks\n" + "".join(gi.mrf_line(CHROM, strands[q] if strands else "+-"[q % 2], file_blocks(r, forward)) for q, r in enumerate(reads))


def candidates1(M, cov):
    """one-block reads from every base of the bucket, ending on, one before, one and two behind every segment end and span
    end, and with the lengths that put the 98 % rule on and beside equality behind every segment end"""
    ends = sorted({t for e in M.events for _, t in e.segs} | {e.ge for e in M.events})
    lo, hi = min(e.gs for e in M.events), max(e.ge for e in M.events)
    out = []
    for a in range(lo, hi):
        bs = {a + 1, a + 40, a + 100}
        for t in ends:
            bs.update((t - 1, t, t + 1, t + 2))
            # 50 x overhang against the length: overhang o behind t, length 50 o - 1, 50 o, 50 o + 1
            for o in (1, 2):
                if t + o - a in (50 * o - 1, 50 * o, 50 * o + 1):
                    bs.add(t + o)
        for b in sorted(bs):
            if 0 < b - a <= 300 and loadable(cov, (a, b)):
                out.append((a, b))
    return out


def candidates2(M, cov):
    """two-block reads: block 1 from a few bases of every cell (first, second, last), ending on / beside every segment end;
    block 2 starting on / one behind every segment start or touching block 1, ending on / beside every segment end and with the
    lengths that put 50 |block 1| against 49 total on and beside equality"""
    ends = sorted({t for e in M.events for _, t in e.segs})
    starts = sorted({s for e in M.events for s, _ in e.segs})
    firsts = sorted({p for c in M.cells for p in (c["lo"], c["lo"] + 1, c["lo"] + 7, c["hi"] - 1) if c["lo"] <= p < c["hi"]}
                    | {e.gs for e in M.events} | {s + 3 for s, t in cov})
    lo, hi = min(e.gs for e in M.events), max(e.ge for e in M.events)
    out = set()
    for t in ends:
        for y in (t - 1, t, t + 1):
            # (block 1 of 48, 49, 50 and 97, 98, 99 bases: with block 2 of 1 / 2 bases 50 |block 1| - 49 total is -1, 0, +1)
            for a in sorted(set(firsts) | {y - ln for ln in (48, 49, 50, 97, 98, 99) if lo <= y - ln < hi}):
                l1 = y - a
                if not 0 < l1 <= 200:
                    continue
                for z in sorted({y} | {s + d for s in starts for d in (0, 1) if s + d > y}):
                    ws = {z + 1, z + 2, z + max(1, l1 // 49), z + l1 // 49 + 1, z + 20, z + 60}
                    for t2 in ends:
                        ws.update((t2 - 2, t2 - 1, t2, t2 + 1))
                    for w in ws:
                        if 0 < w - z <= 200 and loadable(cov, (a, y, z, w)):
                            out.add((a, y, z, w))
    return sorted(out)


def tags(M, rd):
    """Where a read lies against the thresholds that govern it, as (name, offset) pairs with offset -1 / 0 / +1 only:
      e1, e2     a one-block read's end against its cell's two thresholds (start cell: e2 = gene_end - 1)
      mn, mf     ... two-owner cell, past the nearer / farther owner's end where nothing abuts it: 50 x overhang - length
                 (0: the 98 % rule on equality; >= 0: the owner is done with the read)
      m2         ... one-owner cell, past e2: the same figure (the general walk decides there)
      y1, y2     a two-block read's block 1 end against e1, e2;  wg: its end against a start cell's gene_end - 1
      w2, w2b    ... crossing a junction: its end against the end of the junction's second segment / of the one abutting that
      blk        50 |block 1| - 49 total, i.e. |block 1| - 49 |block 2| (0: equality; > 0: block 1 alone can carry the read)
      gs         the read starts on the first base of a span"""
    near = lambda name, v: {(name, v)} if -1 <= v <= 1 else set()
    out = set()
    c = M.cell(rd[0])
    if any(e.gs == rd[0] for e in M.events):
        out.add(("gs", 0))
    if c is None or c["kind"] == "empty":
        return out
    if len(rd) == 2:
        a, b = rd
        out |= near("e1", b - c["e1"]) | near("e2", b - c["e2"])
        if c["kind"] == "two":
            if c["near_free"] and b > c["e1"]:
                out |= near("mn", 50 * (b - c["e1"]) - (b - a))
            if c["far_free"] and b > c["e2"]:
                out |= near("mf", 50 * (b - c["e2"]) - (b - a))
        elif c["kind"] == "one" and b > c["e2"]:
            out |= near("m2", 50 * (b - c["e2"]) - (b - a))
        return out
    a, y, z, w = rd
    if c["kind"] == "start":
        return out | near("wg", w - c["e2"])
    out |= near("y1", y - c["e1"]) | near("y2", y - c["e2"])
    if z != y:
        out |= near("blk", (y - a) - 49 * (w - z))
    j = M.junction(rd)
    if j is not None and z != y:
        ev = M.events[c["owner"][0]]
        end2 = ev.segs[j[2]][1]
        out |= near("w2", w - end2)
        if ev.abuts(j[2]):
            out |= near("w2b", w - ev.segs[j[2] + 1][1])
    return out


def pick(reads, M=None, n_min=300, n_max=360, per_tag=4):
    """at least n_min reads.  With a model: up to per_tag reads of every tag (tags()) are kept whatever else happens -- the
    reads on and beside every threshold and every equality of the 98 % rule --, and only the rest is thinned to an even
    spread.  All of them when they are few (repeated in turn)."""
    reads = sorted(set(reads))
    if not reads:
        return []
    keep = []
    if M is not None:
        by = {}
        for rd in reads:
            for t in tags(M, rd):
                by.setdefault(t, []).append(rd)
        for t in sorted(by):
            rds = by[t]
            keep += [rds[(q * (len(rds) - 1)) // max(per_tag - 1, 1)] for q in range(min(per_tag, len(rds)))]
        keep = sorted(set(keep))
    rest = [rd for rd in reads if rd not in set(keep)]
    room = max(n_max - len(keep), 0)
    if len(rest) > room:
        step = (len(rest) - 1) / max(room - 1, 1)
        rest = [rest[int(round(q * step))] for q in range(room)]
    reads = sorted(set(keep + rest))
    out = list(reads)
    while len(out) < n_min:
        out += reads[:n_min - len(out)]
    return out


def case_files(M, cov):
    """{(verdict, kernel): reads} -- for every kernel and every verdict it has, reads that the model gives that verdict (two-block
    reads: as a lane's first record; "same": J reads of junctions that several reads cross; "by_place" has no file of its own:
    such reads sit in the S_add and drop files)"""
    c1, c2 = candidates1(M, cov), candidates2(M, cov)
    out = {}
    for kernel in cr.KERNELS:
        by = {}
        for rd in c1:
            by.setdefault(cr.verdict1(M, rd, kernel)[0], []).append(rd)
        for rd in c2:
            v = cr.verdict2(M, rd, kernel, "lead")
            by.setdefault(v[0], []).append(rd)
            if v[0] == "J" and cr.verdict2(M, rd, kernel, "follower")[0] == "same":
                by.setdefault("same", []).append(rd)
        # split: cells whose far owners are never near owners of a cell in the file, so that "the farther owner's rows" are whole genes
        if "split" in by:
            far = {M.cell(a)["far"][0] for a, _ in by["split"]}
            by["split"] = [rd for rd in by["split"] if M.cell(rd[0])["near"][0] not in far]
        # same: the reads of every junction repeated, so that every lane leader has followers
        if "same" in by:
            by["same"] = [rd for rd in pick(by["same"], M, 100, 120) for _ in range(2 * cr.PER_LOOK[kernel][1])]
        # park: the reads that cross a junction and run past its segments, each often enough for every lane leader to have
        # followers, beside a spread of all the others
        if "park" in by:
            past = [rd for rd in by["park"] if M.junction(rd) is not None and rd[2] != rd[1]]
            by["park"] = [rd for rd in pick(past, M, 20, 30) for _ in range(2 * cr.PER_LOOK[kernel][1])] + pick(by["park"], M, 300, 320)
        for v, rds in by.items():
            out[(v, kernel)] = pick(rds, M) if v not in ("same", "park") else rds
    return out


def verdict_names(kernel):
    """the verdicts a kernel has, by_place aside (it names no verdict of the loops, only that two of them meet in one read)"""
    return [v for v in cr.VERDICTS1 + cr.VERDICTS2 if v != "by_place" and (kernel != "wide" or v not in cr.COMPACT_ONLY)]


def required_tags(kernel):
    """What every verdict's file must hold (tags()): the reads on its governing threshold and beside it on its own side -- the
    other side is the named neighbour's file -- and, for the verdicts the 98 % rule decides, the read on equality and its
    neighbours.  From the verdicts' definitions, not from what the generator happens to give."""
    compact = kernel != "wide"
    req = {
        "A": {"e1": {-1, 0}},                                   # ends inside the segment: last base but one, last base; +1 is L / split
        "L": {"e1": {1}, "e2": {-1, 0}},                        # (e1, e2]; +1 behind e2 is park_past
        # behind e2; one owner: the walk's 98 % rule on and beside equality; two owners: the farther owner's, which the compact
        # loop decides itself (>= 0: gone) and the wide loop leaves to the walk
        "park_past": {"e2": {1}, "m2": {-1, 0, 1}, "mf": {-1} if compact else {-1, 0, 1}},
        # (e1, e2] of a two-owner cell; past the nearer owner's free end the compact loop parks only below equality (>= 0: far_only)
        "split": {"e1": {1}, "e2": {0}, "mn": {-1} if compact else {-1, 0, 1}},
        "nobody": {"gs": {0}},
        "park_nocell": {"gs": {0}},
        "J": {"w2": {-1, 0}}, "same": {"w2": {-1, 0}},          # block 2 ends inside the junction's second segment; +1 is Jb / park
        "park": {"w2": {1}, "wg": {1}, "y1": {1}},              # past the junction's segment; past a start cell's gene_end - 1; block 1 past e1
        "S_add": {"blk": {1}, "y1": {-1, 0}},                   # block 1 alone carries the read: just above equality
        "S_weak": {"blk": {-1, 0}, "y1": {-1, 0}},              # ... on equality and just below
        "drop": {"gs": {0}, "wg": {-1, 0}},                     # from a start cell, over by gene_end - 1
    }
    if compact:
        req.update({"far_only": {"mn": {0, 1}}, "gone": {"mf": {0, 1}}, "Jb": {"w2": {1}, "w2b": {-1, 0}},
                    "nothing": {"blk": {-1, 0}, "y1": {1}}})
        req["park"]["blk"] = {1}                                # what would be `nothing` one base of block 2 less
    return req
