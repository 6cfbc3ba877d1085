"""A plain model of what the count kernel's streaming loops are SAID to do (test infrastructure; no GPU, no library).

Written from the written definitions -- csrc/lsq_internal.hpp "Shortcut table of a packed bucket", the first-base rule in
csrc/lsq_annot.cpp, the comment blocks ahead of stream_pool_wide, stream_pool1_compact and stream_pool2_compact in
csrc/lsq_count.hip, and the 98 % rule of count/count.cpp:441 -- in terms of events, segments and bases, by brute force
over every base of a small bucket; none of the kernel's arithmetic (bins, thresholds in record terms, packed sums).

    cells(events)                       the cells of a bucket whose events are `events`, in the bucket's order
    verdict1(M, read, kernel)           how a streaming loop settles a one-block read [a, b)
    verdict2(M, read, kernel, place)    ... a two-block read [a, y) [z, w), looked at as a lane's first record ("lead") or as
                                        a later one ("follower"); place None: the verdict where both agree on parking, else
                                        "by_place"
    park_bounds(M, reads, kernel)       how many reads of a file the loops park, from the pools' layout alone

kernel: "wide" (lsq_count_fast_kernel<false, 2>), "compact4" / "compact8" (<true, 2> / <true, 4>: four / eight one-block
reads and two / four two-block reads per lane and look).

A verdict is (name, reason): reason is the index of the developer counter (lsq_debug_counters) that a parked read adds to,
None for a settled one.  The wide loop counts a parked second record in no reason counter (reason None there too)."""

CELL_NO_END = 0x7F000000
CELL_K_START = 63
CELL_INFO_SHARED = 0xFFFFFFFF
CELL_INFO_EMPTY = 0xFFFFFFFE
CELLX_BOTH = 1 << 16
CELLX_NEAR_NO_ABUT = 1 << 17
CELLX_FAR_NO_ABUT = 1 << 18

KERNELS = ("wide", "compact4", "compact8")
# reads a lane takes per look: (one-block, two-block)
PER_LOOK = {"wide": (4, 2), "compact4": (4, 2), "compact8": (8, 4)}
P1_GROUP_PAD, P2_GROUP_PAD = 8, 4

VERDICTS1 = ("A", "L", "split", "far_only", "gone", "nobody", "park_past", "park_nocell")
VERDICTS2 = ("J", "Jb", "S_add", "S_weak", "drop", "nothing", "same", "park", "by_place")
# the verdicts a kernel has (far_only / gone / Jb / nothing: the compact loops only)
COMPACT_ONLY = ("far_only", "gone", "Jb", "nothing")
PARKS = ("split", "park_past", "park_nocell", "park")


class Event:
    """segments ascending (start, end); the span is [first start, last end]"""

    def __init__(self, name, segs):
        self.name = name
        self.segs = [tuple(s) for s in segs]
        self.gs = self.segs[0][0]
        self.ge = max(e for _, e in self.segs)

    def abuts(self, k):
        """segment k + 1 starts where segment k ends"""
        return k + 1 < len(self.segs) and self.segs[k + 1][0] == self.segs[k][1]


def bucket_order(events):
    """the order of a bucket's events: span start, span end, then the order given"""
    return [events[i] for i in sorted(range(len(events)), key=lambda i: (events[i].gs, events[i].ge, i))]


def valid(matched, total):
    """count/count.cpp:441: (double)matched / total > 0.98, in integers"""
    return 50 * matched > 49 * total


def cells(events):
    """The cells of a bucket (events in bucket order), by brute force over every base from the first segment start to the last
    segment end: maximal stretches over which the set of covering segments (event, k) does not change, cut also behind the
    first base of every span.  Each cell is a dict: lo, hi, kind ("start", "empty", "one", "two"), e1, e2 and
      one / start: owner (event, k), at_start (lo is the segment's start)
      two:         near, far (event, k) -- near ends first; on equal ends the one that starts first --, near_free / far_free
                   (no segment abuts that owner's), twin (both owners' segments are the same interval: which is near is open)
    A stretch with more than two owners is no cell, and the first base of a span is none unless the start-cell conditions hold."""
    lo = min(s for e in events for s, _ in e.segs)
    hi = max(t for e in events for _, t in e.segs)
    cuts = {e.gs + 1 for e in events}

    def owners(p):
        return tuple((i, k) for i, e in enumerate(events) for k, (s, t) in enumerate(e.segs) if s <= p < t)

    stretches = []
    for p in range(lo, hi):
        o = owners(p)
        if stretches and stretches[-1][2] == o and p not in cuts:
            stretches[-1][1] = p + 1
        else:
            stretches.append([p, p + 1, o])
    out = []
    for x0, x1, own in stretches:
        starting = [i for i, e in enumerate(events) if e.gs == x0]
        if starting:
            # The first base of a span (lsq_annot.cpp): no cell -- the span-start tie rule decides there -- unless (1) one event
            # only starts here, (2) its first segment is the only cover of the base, (3) the span goes on behind the base: then a
            # start cell, whose reads count for nobody when they end before gene_end
            if len(starting) != 1 or len(own) != 1 or own[0] != (starting[0], 0):
                continue
            e = events[starting[0]]
            if e.ge - 1 < x1:
                continue
            out.append(dict(lo=x0, hi=x1, kind="start", e1=x1, e2=e.ge - 1, owner=own[0], at_start=False))
        elif len(own) == 0:
            out.append(dict(lo=x0, hi=x1, kind="empty", e1=CELL_NO_END, e2=CELL_NO_END))
        elif len(own) == 1:
            i, k = own[0]
            e = events[i]
            e1 = e.segs[k][1]
            out.append(dict(lo=x0, hi=x1, kind="one", e1=e1, e2=e.segs[k + 1][1] if e.abuts(k) else e1, owner=(i, k), at_start=e.segs[k][0] == x0))
        elif len(own) == 2:
            seg = lambda o: events[o[0]].segs[o[1]]
            a, b = sorted(own, key=lambda o: (seg(o)[1], seg(o)[0]))
            out.append(dict(lo=x0, hi=x1, kind="two", e1=seg(a)[1], e2=seg(b)[1], near=a, far=b, twin=seg(a) == seg(b),
                            near_free=not events[a[0]].abuts(a[1]), far_free=not events[b[0]].abuts(b[1])))
    return out


def encode(c):
    """a cell as the library's record: (lo, hi, e1, e2, info, flags)"""
    if c["kind"] == "start":
        info, flags = (c["owner"][0] << 8) | (CELL_K_START << 2), 0
    elif c["kind"] == "empty":
        info, flags = CELL_INFO_EMPTY, 0
    elif c["kind"] == "one":
        info, flags = (c["owner"][0] << 8) | (c["owner"][1] << 2) | (1 if c["at_start"] else 0), 0
    else:
        info = CELL_INFO_SHARED
        flags = CELLX_BOTH | c["far"][0] | (CELLX_NEAR_NO_ABUT if c["near_free"] else 0) | (CELLX_FAR_NO_ABUT if c["far_free"] else 0)
    return (c["lo"], c["hi"], c["e1"], c["e2"], info, flags)


class Model:
    """a bucket: its events in bucket order and their cells, with the cell of every base looked up by position"""

    def __init__(self, events):
        self.events = bucket_order(events)
        self.cells = cells(self.events)
        self.at = {}
        for q, c in enumerate(self.cells):
            for p in range(c["lo"], c["hi"]):
                self.at[p] = q

    def cell(self, p):
        q = self.at.get(p)
        return None if q is None else self.cells[q]

    def junction(self, rd):
        """(cell, variant, segment k2) when the two-block read lies in a junction group of the two-block pool: block 1 starts
        in a one-owner cell and ends on the end of the owner's segment k (variant 0) or of the segment that abuts it (variant
        1), block 2 starts on the first base of a later segment k2 of that event; else None"""
        a, y, z, w = rd
        q = self.at.get(a)
        if q is None or self.cells[q]["kind"] != "one":
            return None
        c = self.cells[q]
        i, k = c["owner"]
        if y == c["e1"]:
            v = 0
        elif y == c["e2"]:
            v = 1
        else:
            return None
        for k2 in range(k + v + 1, len(self.events[i].segs)):
            if self.events[i].segs[k2][0] == z:
                return (q, v, k2)
        return None

    def group2(self, rd):
        """the group of the two-block pool a read lies in: a lane's records of one look come from one group"""
        j = self.junction(rd)
        return ("j",) + j[:2] + (rd[2],) if j else ("c", self.at.get(rd[0]))


def verdict1(M, rd, kernel):
    """a one-block read [a, b) against the cell its first base lies in (a lane's records of one look start in one cell)"""
    a, b = rd
    c = M.cell(a)
    if c is None:
        return ("park_nocell", 5)
    if c["kind"] == "empty":
        return ("nobody", None)
    if c["kind"] == "start":
        return ("nobody", None) if b <= c["e2"] else ("park_past", 6)
    if c["kind"] == "one":
        if b <= c["e1"]:
            return ("A", None)
        return ("L", None) if b <= c["e2"] else ("park_past", 6)
    if b <= c["e1"]:
        return ("A", None)
    if kernel == "wide":
        return ("split", 7) if b <= c["e2"] else ("park_past", 7)
    # the compact loop: past the end of an owner's segment that nothing abuts the read matches that owner up to the end only,
    # and when that is no more than 98 % of it the owner is done with the read.
    # (near_done / far_done restate the kernel's own claim, term for term -- they are no independent derivation.  What makes
    # the claim true or false is the oracle: a `gone` file must come out all zero there, a `far_only` file equal to the
    # loops-alone table.  The model only picks the reads and says how many of them are parked.)
    near_done = c["near_free"] and not valid(c["e1"] - a, b - a)
    far_done = b <= c["e2"] or (c["far_free"] and not valid(c["e2"] - a, b - a))
    if b <= c["e2"]:
        return ("far_only", None) if near_done else ("split", 7)
    return ("gone", None) if near_done and far_done else ("park_past", 7)


def _weak(rd):
    """block 1 alone cannot carry the read (and the blocks do not touch: the exception pass decides those)"""
    a, y, z, w = rd
    return z != y and not valid(y - a, (y - a) + (w - z))


def _nothing(M, rd):
    """a record of a group that crosses no junction, settled as counting for nobody by the compact two-block loop.
    (This restates the kernel's `nothing` term for term -- its claim of when block 1 alone bounds what any owner can match --,
    not an independent derivation: the claim is judged by the oracle, whose table of a `nothing` file must be all zero.)"""
    a, y, z, w = rd
    c = M.cell(a)
    if c is None:
        return False
    if c["kind"] == "empty":
        return True
    if not _weak(rd):
        return False
    if c["kind"] == "two":
        return y != c["e1"] and y != c["e2"] and (y < c["e1"] or c["near_free"]) and (y < c["e2"] or c["far_free"])
    return c["kind"] == "one" and y <= c["e2"]


def verdict2(M, rd, kernel, place):
    a, y, z, w = rd
    if place is None:
        vl, vf = verdict2(M, rd, kernel, "lead"), verdict2(M, rd, kernel, "follower")
        return vl if (vl[0] in PARKS) == (vf[0] in PARKS) else ("by_place", None)
    c = M.cell(a)
    j = M.junction(rd)
    touching = z == y
    if j is not None and not touching:
        ev = M.events[c["owner"][0]]
        end2 = ev.segs[j[2]][1]
        end2b = ev.segs[j[2] + 1][1] if ev.abuts(j[2]) else end2
    if place == "follower":
        if kernel == "wide":
            # no look of its own: the first record's junction or nothing
            return ("same", None) if j is not None and j[1] == 0 and not touching and w <= end2 else ("park", None)
        if j is not None and not touching:
            return ("same", None) if w <= end2b else ("park", 14)
        return ("nothing", None) if _nothing(M, rd) else ("park", 13)
    if c is None:
        return ("park", 8)
    if c["kind"] == "empty":
        return ("drop", None)
    if c["kind"] == "start":
        return ("drop", None) if w <= c["e2"] else ("park", 9)
    if c["kind"] == "two":
        return ("nothing", None) if kernel != "wide" and _nothing(M, rd) else ("park", 8)
    if touching:
        return ("park", 9)
    if j is not None and (kernel != "wide" or j[1] == 0):
        if w <= end2:
            return ("J", None)
        return ("Jb", None) if kernel != "wide" and w <= end2b else ("park", 9)
    if y <= c["e1"]:
        return ("S_add", None) if valid(y - a, (y - a) + (w - z)) else ("S_weak", None)
    return ("nothing", None) if kernel != "wide" and _nothing(M, rd) else ("park", 9)


def park_bounds(M, reads, kernel):
    """What the loops park of a file, from the pools' layout alone (the order of a group's records is not defined).
    Returns dict(parked1, reasons1 {5, 6, 7}, parked2 (lo, hi), reasons2 {8, 9, 13, 14} or None where the records' order decides,
    looks (the two-block looks: lane leaders), by_place (two-block reads whose parking depends on their place))."""
    r1 = {5: 0, 6: 0, 7: 0}
    groups = {}
    for rd in reads:
        if len(rd) == 2:
            v = verdict1(M, rd, kernel)
            if v[1] is not None:
                r1[v[1]] += 1
        else:
            groups.setdefault(M.group2(rd), []).append(rd)
    per = PER_LOOK[kernel][1]
    lo = hi = by_place = looks = 0
    r2 = {8: 0, 9: 0, 13: 0, 14: 0}
    exact = True
    for g, rds in groups.items():
        n = len(rds)
        lead = (n + per - 1) // per
        looks += lead
        kinds = set()
        pp = np_ = 0
        for rd in rds:
            vl, vf = verdict2(M, rd, kernel, "lead"), verdict2(M, rd, kernel, "follower")
            pl, pf = vl[0] in PARKS, vf[0] in PARKS
            assert pf or not pl, ("a record parked as a lane's first and settled behind one", rd, vl, vf)
            pp += pl and pf
            np_ += pf and not pl
            kinds.add((pl, pf, vl[1], vf[1]))
        by_place += np_
        lo += pp + max(0, np_ - lead)
        hi += pp + min(np_, n - lead)
        if len(kinds) == 1:
            pl, pf, rl, rf = next(iter(kinds))
            if pl and rl is not None:
                r2[rl] += lead
            if pf and rf is not None:
                r2[rf] += n - lead
        else:
            exact = False
    return dict(parked1=sum(r1.values()), reasons1=r1, parked2=(lo, hi), reasons2=r2 if exact else None, looks=looks, by_place=by_place)


def looks_of_walk(M, p):
    """the events the general walk looks at for a read that starts at p and was parked without an event to look at: from the
    first event whose span has not ended left of p, on while the event looked at has ended left of p or the next one starts
    inside its span.  (For a bucket all of whose spans reach p: the chain from its first event.)"""
    ev = M.events
    i = 0
    while i < len(ev) and ev[i].ge < p:
        i += 1
    n = 0
    while i < len(ev):
        n += 1
        started = ev[i].gs <= p
        more = started and (not p <= ev[i].ge or (i + 1 < len(ev) and ev[i + 1].gs <= ev[i].ge)) and i + 1 < len(ev)
        if not more:
            break
        i += 1
    return n
