"""Expected tables of the stranded read-file tools.  Not a test module.

A stranded table is by definition two unstranded tables: that of the plus genes / events alone on the reads whose transcript
strand t is "+", and that of the minus ones alone on the reads with t = "-", the rows put back in the order the unstranded table of
the whole annotation has.  So the expected values come from the tools' own brute-force references (exonbins_ref, psi_ref, evidence_ref), run
twice on inputs split here in Python: nothing of the library is involved.  A read that is left out of a split file becomes a '#'
line, so every read keeps its line number."""
import stranded_inputs as S

LIBRARY_REPORT = ("plus", "minus", "no_strand", "plus_counted", "minus_counted")
# the report entries that are the unstranded run's on the whole annotation; every other entry is the sum of the two split runs'
READ_LEVEL = {"exonbins_ref": ("reads", "blocks", "no_chromosome_or_empty"),
              "psi_ref": ("reads", "blocks", "occurrences", "dropped_overhang", "no_chromosome"),
              "evidence_ref": ("reads", "blocks", "occurrences", "dropped_overhang", "no_chromosome", "skipped_blocks")}
# reads of a split run that counted for at least one of its genes / events, from its report
COUNTED = {"exonbins_ref": lambda rep: rep["reads"] - rep["no_gene"], "psi_ref": lambda rep: rep["counted"], "evidence_ref": lambda rep: rep["counted"]}


def annotation_texts(genes):
    """(interval text, map text) as stranded_inputs.write_annotation writes them"""
    iv, mp = [], []
    for ge in genes:
        for iname, exons in ge.isoforms:
            st = ge.strand if isinstance(ge.strand, str) else ge.strand[iname]
            iv.append("%s\t%s\t%s\t%d\t%d\t%d\t%s\t%s\n" % (iname, ge.chrom, st, exons[0][0], exons[-1][1], len(exons),
                                                           ",".join(str(s) for s, _ in exons), ",".join(str(e) for _, e in exons)))
            mp.append("%s\t%s\n" % (ge.name, iname))
    return "".join(iv), "".join(mp)


def unstranded(tool_ref, genes, recs, n_comment=len(S.SAM_HEADER), table=None, **kw):
    """the reference's table of the whole annotation on all reads, whatever their strand: what the tools give without a library type"""
    iv, mp = annotation_texts(genes)
    return (table or tool_ref.table)(iv, mp, S.input_mrf(recs, n_comment), **kw)


def expected(tool_ref, genes, recs, lib, n_comment=len(S.SAM_HEADER), table=None, **kw):
    """(want, library report): `want` is what tool_ref.table returns -- rows, report and whatever follows them -- for the stranded
    table; table: another function of the reference's with table()'s arguments and result (its numpy form, where it has one)"""
    table = table or tool_ref.table
    name = tool_ref.__name__
    whole = unstranded(tool_ref, genes, recs, n_comment, table, **kw)
    parts = []
    for tbit, strand in enumerate("+-"):
        iv, mp = annotation_texts([g for g in genes if g.strand == strand])
        parts.append(table(iv, mp, S.mrf_text(recs, n_comment, lambda r: strand if r.t(lib) == tbit else None), **kw))
    by_id = {}
    for p in parts:
        for row in p[0]:
            assert (row[0], row[2]) not in by_id
            by_id[(row[0], row[2])] = row
    rows = [by_id[(row[0], row[2])] for row in whole[0]]
    assert len(rows) == len(by_id)
    report = {k: whole[1][k] if k in READ_LEVEL[name] else parts[0][1][k] + parts[1][1][k] for k in whole[1]}
    t = [r.t(lib) for r in recs]
    assert [p[1]["reads"] for p in parts] == [t.count(0), t.count(1)] and whole[1]["reads"] == len(recs)
    lib_report = dict(zip(LIBRARY_REPORT, (t.count(0), t.count(1), t.count(None), COUNTED[name](parts[0][1]), COUNTED[name](parts[1][1]))))
    return (rows, report) + tuple(whole[2:]), lib_report


# ----------------------------------------------------------------------------- libtype: which library type is this file?

LIM = 1 << 30
LIBTYPE_KEYS = ("reads", "no_strand", "plus_none", "plus_plus", "plus_minus", "plus_both", "minus_none", "minus_plus", "minus_minus", "minus_both",
                "sense", "antisense", "ambiguous", "no_gene", "unplaced_genes")


def libtype(genes, recs):
    """The counts of `libtype` by brute force: every block of every read against every exon of every gene.  A gene has a strand
    when all its isoform lines carry the same one of + / -; the others are left out and counted.  A read has r = s XOR mate2 of
    its first block (stranded_inputs.Rec.r_minus), or none where an MRF strand column is neither + nor -."""
    known = {g.chrom for g in genes}
    exons = {"+": [], "-": []}
    unplaced = 0
    for g in genes:
        strands = {g.strand} if isinstance(g.strand, str) else set(g.strand.values())
        if len(strands) != 1 or next(iter(strands)) not in ("+", "-"):
            unplaced += 1
            continue
        exons[next(iter(strands))] += [(g.chrom, s, e) for _, ex in g.isoforms for s, e in ex if e > s]
    c = dict.fromkeys(LIBTYPE_KEYS, 0)
    c["reads"], c["unplaced_genes"] = len(recs), unplaced
    for r in recs:
        if r.mrf_strand is not None and r.mrf_strand not in ("+", "-"):
            c["no_strand"] += 1
            continue
        chroms = getattr(r, "chroms", [r.chrom] * len(r.blocks))
        blocks = [(ch, s, e) for ch, (s, e) in zip(chroms, r.blocks) if ch in known and e > s and -LIM < s < LIM and -LIM < e < LIM]
        on = {st: any(ch == gc and s < ge and e > gs for ch, s, e in blocks for gc, gs, ge in exons[st]) for st in "+-"}
        c[("minus_" if r.r_minus else "plus_") + ("both" if on["+"] and on["-"] else "plus" if on["+"] else "minus" if on["-"] else "none")] += 1
    c["sense"] = c["plus_plus"] + c["minus_minus"]
    c["antisense"] = c["plus_minus"] + c["minus_plus"]
    c["ambiguous"] = c["plus_both"] + c["minus_both"]
    c["no_gene"] = c["plus_none"] + c["minus_none"]
    return c


def libtype_verdict(c):
    """(forward_fraction or None, library) by the fixed conventions"""
    n = c["sense"] + c["antisense"]
    f = c["sense"] / n if n else None
    if n < 100:
        return f, "undetermined"
    return f, "forward" if f >= 0.9 else "reverse" if f <= 0.1 else "unstranded" if 0.4 <= f <= 0.6 else "undetermined"


def libtype_text(c):
    f, lib = libtype_verdict(c)
    return "".join("%s\t%d\n" % (k, c[k]) for k in LIBTYPE_KEYS) + "forward_fraction\t%s\nlibrary\t%s\n" % ("NA" if f is None else "%.6f" % f, lib)
