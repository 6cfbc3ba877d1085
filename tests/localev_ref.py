"""An independent restatement of bin/Events.r in Python (line numbers cite the script), and a deterministic generator of
gene models with every local-event shape planted.  Used by tests/test_localevents_*.py and tools/events_bench.py."""
import os
import random
import re

TYPES = ("ES", "RI", "A5SS", "A3SS", "MXE", "AFE", "ALE", "T3")


def r_double(v):
    """as.character of a whole-number double (the counters): scientific when strictly shorter (1e+05)"""
    s = "%d" % v
    m = s.rstrip("0")
    z = len(s) - len(m)
    if z:
        sci = m[0] + ("." + m[1:] if len(m) > 1 else "") + "e+%02d" % (len(s) - 1)
        if len(sci) < len(s):
            return sci
    return s


def read_matrix(path):
    """(chr, strand, pos, rows) as Events.r:49-55 reads them"""
    with open(path) as f:
        lines = f.read().split("\n")
    head = lines[0].split("\t")
    digits = "".join(c if c.isdigit() else " " for c in head[2])
    # strsplit(..., " {1,}") gives no trailing empty piece; [-1] drops the first (the "" before a leading non-digit)
    pieces = re.split(" +", digits)
    if pieces and pieces[-1] == "":
        pieces.pop()
    pos = [int(x) for x in pieces[1:]]
    rows = [[int(x) for x in ln.split()] for ln in lines[1:] if ln.strip()]
    return head[0], head[1], pos, rows


def events_of_gene(gid, chr_, strand, pos, rows):
    """{type: [(iv_line1, iv_line2)]} for one gene (Events.r:57-156)"""
    out = {t: [] for t in TYPES}
    ncol = len(rows[0])
    if ncol < 3:                                           # :57
        return out
    K = len(rows)
    usage = [None] + [sum(r[c] for r in rows) for c in range(ncol)]     # 1-based
    col = [None] + [[r[c] for r in rows] for c in range(ncol)]
    P = [None] + pos                                       # pos[j], 1-based
    k = len(pos)
    N = ncol

    def comp(a, b):
        return all(x != y for x, y in zip(col[a], col[b]))

    def line(tag, w, s, e, n, starts, ends):
        return "\t".join([gid + "|" + str(tag) + "|" + str(w), chr_, strand, str(s), str(e), str(n),
                          ",".join(map(str, starts)), ",".join(map(str, ends))])

    def loop_pair(i):
        return (line(i, 1, P[i*2-3], P[i*2+2], 3, [P[i*2-3], P[i*2-1], P[i*2+1]], [P[i*2-2], P[i*2], P[i*2+2]]),
                line(i, 2, P[i*2-3], P[i*2+2], 2, [P[i*2-3], P[i*2+1]], [P[i*2-2], P[i*2+2]]))

    for i in range(2, N):                                  # :62-93
        if K == usage[i-1] and K == usage[i+1] and K > usage[i]:
            gl, gr = P[i*2-1] - P[i*2-2], P[i*2+1] - P[i*2]
            if gl > 0 and gr > 0:
                out["ES"].append(loop_pair(i))
            if gl == 0 and gr == 0:
                out["RI"].append(loop_pair(i))
            if (strand == "+" and gl == 0 and gr > 0) or (strand == "-" and gl > 0 and gr == 0):
                out["A5SS"].append(loop_pair(i))
            if (strand == "+" and gl > 0 and gr == 0) or (strand == "-" and gl == 0 and gr > 0):
                out["A3SS"].append(loop_pair(i))
    if N >= 4:                                             # :95-107
        for i in range(4, N + 1):
            if K == usage[i-3] and K == usage[i] and comp(i-2, i-1):
                if P[i*2-1] - P[i*2-2] > 0 and P[i*2-3] - P[i*2-4] > 0 and P[i*2-5] - P[i*2-6] > 0:
                    out["MXE"].append((line(i, 1, P[i*2-7], P[i*2], 3, [P[i*2-7], P[i*2-5], P[i*2-1]], [P[i*2-6], P[i*2-4], P[i*2]]),
                                       line(i, 2, P[i*2-7], P[i*2], 3, [P[i*2-7], P[i*2-3], P[i*2-1]], [P[i*2-6], P[i*2-2], P[i*2]])))
    if K == usage[3] and comp(1, 2) and P[3] - P[2] > 0 and P[5] - P[4] > 0:      # :109-124
        tag = {"+": "AFE", "-": "ALE"}.get(strand)
        if tag:
            out[tag].append((line(tag, 1, P[3], P[6], 2, [P[3], P[5]], [P[4], P[6]]),
                             line(tag, 2, P[1], P[6], 2, [P[1], P[5]], [P[2], P[6]])))
    if K == usage[N-2] and comp(N-1, N) and P[k-1] - P[k-2] > 0 and P[k-3] - P[k-4] > 0:   # :126-141
        tag = {"+": "ALE", "-": "AFE"}.get(strand)
        if tag:
            out[tag].append((line(tag, 1, P[k-5], P[k-2], 2, [P[k-5], P[k-3]], [P[k-4], P[k-2]]),
                             line(tag, 2, P[k-5], P[k], 2, [P[k-5], P[k-1]], [P[k-4], P[k]])))
    if strand == "+" and K == usage[N-1] and K > usage[N] and P[k-1] - P[k-2] == 0:      # :143-149
        out["T3"].append((line("T3", 1, P[k-3], P[k], 1, [P[k-3]], [P[k]]), line("T3", 2, P[k-3], P[k-2], 1, [P[k-3]], [P[k-2]])))
    if strand == "-" and K == usage[2] and K > usage[1] and P[3] - P[2] == 0:           # :150-156
        out["T3"].append((line("T3", 1, P[1], P[4], 1, [P[1]], [P[4]]), line("T3", 2, P[3], P[4], 1, [P[3]], [P[4]])))
    return out


def gene_ids(group_path):
    """Events.r:40-42 for the id forms these tests use: all integers -> numeric order; otherwise byte order"""
    ids = [ln.split()[0] for ln in open(group_path).read().split("\n") if ln.strip()]
    if all(x.lstrip("+-").isdigit() for x in ids):
        keys = [int(x) for x in ids]
        cnt = {}
        for x in keys:
            cnt[x] = cnt.get(x, 0) + 1
        return [str(x) for x in sorted(cnt) if cnt[x] > 1]
    cnt = {}
    for x in ids:
        cnt[x] = cnt.get(x, 0) + 1
    return sorted((x for x in cnt if cnt[x] > 1), key=lambda s: s.encode())


def events_files(prefix, group_path):
    """(stdout, {file name: text}) that Events.r writes for a fresh out_prefix"""
    stdout = []
    iv = {t: [] for t in TYPES}
    mp = {t: [] for t in TYPES}
    for gid in gene_ids(group_path):
        stdout.append('[1] "processing gene: %s"\n' % gid.replace("\\", "\\\\").replace('"', '\\"'))
        chr_, strand, pos, rows = read_matrix(prefix + gid + ".matrix")
        for t, evs in events_of_gene(gid, chr_, strand, pos, rows).items():
            for a, b in evs:
                c = r_double(len(mp[t]) // 2 + 1)
                iv[t] += [a + "\n", b + "\n"]
                mp[t] += ["%s\t%s\n" % (c, a.split("\t")[0]), "%s\t%s\n" % (c, b.split("\t")[0])]
    files = {}
    for t in TYPES:
        if iv[t]:
            files[t + ".interval"] = "".join(iv[t])
            files[t + ".map"] = "".join(mp[t])
    return "".join(stdout), files


def read_out(prefix):
    d, stem = os.path.split(prefix)
    out = {}
    for fn in sorted(os.listdir(d or ".")):
        if fn.startswith(stem) and fn[len(stem):].split(".")[0] in TYPES:
            out[fn[len(stem):]] = open(os.path.join(d, fn)).read()
    return out


# ----------------------------------------------------------------------------- generator

def _iline(name, chrom, strand, exons):
    exons = sorted(exons)
    return "%s\t%s\t%s\t%d\t%d\t%d\t%s\t%s\n" % (name, chrom, strand, exons[0][0], exons[-1][1], len(exons),
                                              ",".join(str(s) for s, _ in exons), ",".join(str(e) for _, e in exons))


def gene_models(n_genes, seed=1, wide_every=2000, wide_shapes=((80, 20), (8, 70))):
    """Deterministic gene models: [(gene id, [(isoform, chrom, strand, exons)])].  Skipped exons (the bulk: ES), alternative
    5' / 3' ends and retained introns (abutting segments: A5SS, A3SS, RI), mutually exclusive pairs, alternative first /
    last exons, alternative terminal starts / ends (T3); strands + - and '.'; small genes (N = 3, 4); every `wide_every`
    genes one of the wide shapes (exons, isoforms) in turn: by default one with N > 64 and one with K > 64."""
    rng = random.Random(seed)
    genes = []
    for g in range(n_genes):
        chrom = "chr%d" % (1 + g % 7)
        strand = "+-+-."[g % 5]
        base = 1000 + 40000 * (g // 7)
        if wide_every and g % wide_every == wide_every - 1:
            E, n_iso = wide_shapes[(g // wide_every) % len(wide_shapes)]
        else:
            E = rng.choice((3, 4, 5, 6, 8, 10, 12, 16, 20, 24))
            n_iso = None
        ex = [(base + 300 * j, base + 300 * j + 100 + rng.randrange(0, 60)) for j in range(E)]
        isos = [list(ex)]
        # one isoform per skipped interior exon (every other one: a skip next to a skip is no ES)
        for j in range(1, E - 1, 2):
            isos.append([e for q, e in enumerate(ex) if q != j])
        r = rng.random()
        if r < 0.15 and E >= 3:                            # alternative 5' / 3' end of an interior exon
            j = rng.randrange(1, E - 1)
            s, e = ex[j]
            alt = list(ex)
            alt[j] = (s - 40, e) if rng.random() < 0.5 else (s, e + 40)
            isos.append(alt)
        elif r < 0.22 and E >= 3:                          # retained intron
            j = rng.randrange(0, E - 1)
            alt = ex[:j] + [(ex[j][0], ex[j + 1][1])] + ex[j + 2:]
            isos.append(alt)
        elif r < 0.32 and E >= 4:                          # mutually exclusive pair j, j+1
            j = rng.randrange(1, E - 2)
            isos = [[e for q, e in enumerate(ex) if q != j + 1], [e for q, e in enumerate(ex) if q != j]]
        elif r < 0.42 and E >= 4:                          # alternative first exons / last exons
            if rng.random() < 0.5:
                isos = [[e for q, e in enumerate(ex) if q != 1], ex[1:]]
            else:
                isos = [[e for q, e in enumerate(ex) if q != E - 2], ex[:E - 1]]
        elif r < 0.50:                                     # alternative terminal start / end abutting the next segment
            alt = list(ex)
            if rng.random() < 0.5:
                alt[-1] = (ex[-1][0], ex[-1][1] + 50)
            else:
                alt[0] = (ex[0][0] - 50, ex[0][1])
            isos.append(alt)
        if n_iso:
            while len(isos) < n_iso:
                j = rng.randrange(1, E - 1)
                alt = [e for q, e in enumerate(ex) if q != j]
                if rng.random() < 0.5:                     # and an alternative end: more atomic segments
                    q = rng.randrange(1, len(alt) - 1)
                    alt[q] = (alt[q][0], alt[q][1] + rng.randrange(5, 60))
                isos.append(alt)
        if len(isos) < 2:
            isos.append(list(ex[:1] + ex[2:]) if E >= 3 else list(ex))
        genes.append(("G%06d" % g, [("G%06d.%d" % (g, q), chrom, strand, iso) for q, iso in enumerate(isos)]))
    return genes


def write_models(genes, d, stem):
    iv, mp = [], []
    for gid, isos in genes:
        for name, chrom, strand, exons in isos:
            iv.append(_iline(name, chrom, strand, exons))
            mp.append("%s\t%s\n" % (gid, name))
    with open(os.path.join(d, stem + ".interval"), "w") as f:
        f.writelines(iv)
    with open(os.path.join(d, stem + ".map"), "w") as f:
        f.writelines(mp)
    return os.path.join(d, stem + ".interval"), os.path.join(d, stem + ".map")
