"""The routing reference (tests/route_ref.py) pinned without a GPU: against reads worked out by hand, against the oracle on every
case file of tests/test_route_gpu.py, and the case files against what they claim to contain."""
import pytest

import lesseq_amd as L
import oracle_binding as ob
import route_ref as rr


def compiled(case, d, library=None):
    iv, mp, paths = case.write(str(d))
    ev = L.Events(L.Annotation(iv, mp), ("SHORT_READ",), (50,), library=library or case.library)
    return iv, mp, paths, ev


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    out = {}
    for case in rr.all_cases():
        iv, mp, paths, ev = compiled(case, tmp_path_factory.mktemp(case.name))
        out[case.name] = (case, iv, mp, paths, ev, rr.Job(ev, case.chroms))
    return out


# exons: G on chr1 [100,200) [300,400) [500,600); H on chr2 [1000,1100) [1200,1300)
HAND_GENES = [("G", "chr1", "+", [[(100, 200), (300, 400), (500, 600)], [(100, 200), (500, 600)]]),
              ("H", "chr2", "+", [[(1000, 1100), (1200, 1300)], [(1000, 1100)]])]
HAND = [
    # (blocks of the line, expected: None = not retained, else (chromosome, strand, merged blocks, genes with the first base in their span))
    ([("chr1", 120, 160)], ("chr1", "+", ((120, 160),), ["G"])),                                          # kept whole
    ([("chr1", 100, 200)], ("chr1", "+", ((100, 200),), ["G"])),                                          # a whole region
    ([("chr1", 100, 201)], None),                                                                        # one base too many
    ([("chr1", 99, 150), ("chr1", 310, 350)], ("chr1", "+", ((310, 350),), ["G"])),                       # dropped on the left of a region
    ([("chr1", 150, 201), ("chr1", 310, 350)], ("chr1", "+", ((310, 350),), ["G"])),                      # ... on the right
    ([("chr1", 120, 140), ("chr1", 140, 160)], ("chr1", "+", ((120, 160),), ["G"])),                      # begins where the other ends: one block
    ([("chr1", 140, 160), ("chr1", 120, 140)], ("chr1", "+", ((120, 140), (140, 160)), ["G"])),           # ends where the other begins: two
    ([("chr1", 120, 140), ("chr1", 310, 330), ("chr1", 130, 150)], ("chr1", "+", ((120, 150), (310, 330)), ["G"])),      # three kept, two left
    ([("chr1", 120, 130), ("chr1", 150, 160), ("chr1", 125, 155)], ("chr1", "+", ((120, 160),), ["G"])),  # a bridge: 2 -> 1
    ([("chr1", 110, 130), ("chr1", 100, 110), ("chr1", 120, 140)], ("chr1", "+", ((100, 110), (110, 140)), ["G"])),      # file order, not sorted order (sorted: one block)
    ([("chr1", 120, 140), ("chr1", 700, 700, "-")], ("chr1", "-", ((120, 140),), ["G"])),                 # an empty last block: its strand
    ([("chr1", 120, 140), ("chr2", 1010, 1050)], ("chr2", "+", ((120, 140), (1010, 1050)), [])),          # two chromosomes: the last one's, where 120 is in no span
    ([("chr2", 1010, 1050), ("chr1", 120, 140)], ("chr1", "+", ((120, 140), (1010, 1050)), ["G"])),
    ([("chr1", 250, 260)], None),                                                                        # between two regions
    ([("chr1", 250, 250)], None),                                                                        # kept, and empty
    ([("chr9", 120, 160)], None),                                                                        # a chromosome without tables
    ([("chr1", 599, 600)], ("chr1", "+", ((599, 600),), ["G"])),                                          # the span's last base
    ([("chr2", 1299, 1300), ("chr2", 1300, 1301)], ("chr2", "+", ((1299, 1300),), ["H"])),
]


def test_hand_table(tmp_path):
    case = rr.Case("hand", HAND_GENES, ("chr1", "chr2", "chr9"), {"r": rr.text_of([b for b, _ in HAND])})
    iv, mp, paths, ev = compiled(case, tmp_path)
    job = rr.Job(ev, case.chroms)
    assert job.regions("chr1", 0) == [(100, 200), (300, 400), (500, 600)] and job.regions("chr2", 0) == [(1000, 1100), (1200, 1300)]
    reads, tally = rr.route(job, case.texts["r"])
    for k, (_, want) in enumerate(HAND, 1):
        if want is None:
            assert k not in reads, (k, reads[k].blocks if k in reads else None)
            continue
        r = reads[k]
        assert (r.chrom, r.strand, r.blocks, [ev.gene_name(i) for i in r.must]) == want, k
    assert (tally["lines"], tally["dropped"], tally["only_empty"]) == (len(HAND), 3, 1)
    assert reads[12].may == [] and [ev.gene_name(i) for i in reads[18].may] == ["H"]
    # the text's own rules: a header whatever it says, '#' lines and a repeated header keep their numbers
    assert [k for k, _ in rr.parse_mrf("x\n#c\nchr1:+:1:2:1:2\nAlignmentBlocks\nchr1:+:-4:0:1:5,chr1:-:7:9:6:8\n")] == [2, 4]
    assert rr.parse_mrf("x\nchr1:+:-4:0:1:5,chr1:-:7:9:6:8\n")[0][1] == [("chr1", "+", -5, 0), ("chr1", "-", 6, 9)]


def split_by_strand(job, text, tbit):
    """the lines of a stranded job's text whose transcript strand is tbit, the others as '#' lines (stranded_inputs: a stranded
    job is two unstranded ones)"""
    lines = text.split("\n")
    for k in range(1, len(lines)):
        if lines[k] and not lines[k].startswith("#"):
            s0 = lines[k].split(":")[1]
            if s0 not in ("+", "-") or int((s0 == "-") ^ (job.library == "reverse")) != tbit:
                lines[k] = "#"
    return "\n".join(lines)


@pytest.mark.parametrize("name", [c.name for c in rr.all_cases()])
def test_reference_agrees_with_the_oracle(name, cases, tmp_path):
    """n_loaded is the reference's retained reads (a read whose kept blocks are all empty is in neither), and no event counts a
    read that the reference puts outside its closed window"""
    case, iv, mp, paths, ev, job = cases[name]
    for stem, text in case.texts.items():
        reads, tally = rr.route(job, text)
        runs = []
        if not job.stranded:
            runs.append((iv, mp, paths[stem], len(reads), None))
        else:
            for tbit, strand in enumerate("+-"):
                sub = rr.Case("%s_%d" % (name, tbit), [g for g in case.genes if g[2] == strand], case.chroms, {stem: split_by_strand(job, text, tbit)})
                siv, smp, sp = sub.write(str(tmp_path))
                runs.append((siv, smp, sp[stem], tally["kept_minus" if tbit else "kept_plus"], strand))
        for riv, rmp, rpath, n_retained, strand in runs:
            rc, _, exact = ob.run("count", case.argv(riv, rmp, rpath))
            assert rc == 0 and ob.last_n_loaded[0] == n_retained, (name, stem, strand, ob.last_n_loaded, n_retained)
            in_window = set(i for r in reads.values() for i in r.may)
            by_name = {ev.gene_name(i): i for i in range(len(ev))}
            n_counted = 0
            for g in exact:
                n_counted += g["supports"][0]
                if by_name[g["gname"]] not in in_window:
                    assert g["supports"] == [0], (name, stem, g["gname"])
            assert n_counted <= sum(len(r.may) for r in reads.values())


@pytest.mark.parametrize("name", [c.name for c in rr.all_cases()])
def test_case_files_contain_what_they_claim(name, cases):
    case, iv, mp, paths, ev, job = cases[name]
    for c in case.chroms:                      # the case builders' idea of the covered regions is the events'
        for t, strand in enumerate("+-" if job.stranded else (None,)):
            assert job.regions(c, t) == rr.regions_of(case.genes, c, strand), (name, c, strand)
    for stem, text in case.texts.items():
        reads, tally = rr.route(job, text)
        rr.assert_contains(case, stem, rr.outcomes(job, reads, tally))
    if name == "shard":
        assert [ev.gene_name(i)[:2] for i in range(len(ev))] == ["g0"] * 5 + ["g1"] * 5
        for q, sh in enumerate(((0, 5), (5, 5))):
            j2 = rr.Job(ev, case.chroms, shard=sh)
            reads, tally = rr.route(j2, case.texts["r"])
            rr.assert_contains(case, "r", rr.outcomes(j2, reads, tally), rr.WANT_SLICE + (("closed_only",) if q == 0 else ()))
    if name == "stranded":
        assert job.regions("chrS", 0) != job.regions("chrS", 1) and job.regions("chrT", 1) == []
        rev = rr.Job(L.Events(L.Annotation(iv, mp), ("SHORT_READ",), (50,), library="reverse"), case.chroms)
        f, r = rr.route(job, case.texts["r"]), rr.route(rev, case.texts["r"])
        assert f[1]["made_plus"] == r[1]["made_minus"] and f[1]["kept_plus"] != r[1]["kept_minus"] and r[1]["kept_plus"] >= 1 and r[1]["kept_minus"] >= 1


def test_bins_case_reaches_both_branches_of_both_searches(cases):
    """shift 10; bins of 0, 1, 3, 4, 5 and >= 9 region starts and of >= 5 span starts: with at most three starts in a bin a search
    is five loads, with more it is a binary search -- both for the covered regions and for the clusters"""
    case, iv, mp, paths, ev, job = cases["bins"]
    assert rr.shift_of(job, case.chroms) == 10
    base, nb = rr.locator_of(job, "chrA")
    assert base == 10240 == min(s for s, _ in job.regions("chrA", 0))                     # on a multiple of 1 024 ...
    assert rr.locator_of(job, "chrB")[0] < min(s for s, _ in job.regions("chrB", 0))      # ... and off one
    assert rr.locator_of(job, "chrD")[0] < 0 and sum(1 for i in job.planned if job.ev[i][0] == "chrC") == 1
    cov = rr.starts_per_bin([s for s, _ in job.regions("chrA", 0)], base, nb)
    spans = rr.starts_per_bin([job.ev[i][2] for i in job.planned if job.ev[i][0] == "chrA"], base, nb)
    assert set(cov) >= {0, 1, 3, 4, 5} and max(cov) >= 9 and max(spans) >= 5
    # blocks on, before and behind every bin edge, before bin 0 and behind the last bin
    starts = set(b[2] for _, bl in rr.parse_mrf(case.texts["r"]) for b in bl if b[0] == "chrA")
    for k in range(-1, nb + 2):
        assert {base + 1024 * k - 1, base + 1024 * k, base + 1024 * k + 1} <= starts, k


def test_wide_cases_sit_on_either_side_of_the_grid_cap(cases):
    for name, entries, shift in (("wide4", 4191412, 10), ("wide5", 5239265, 11)):
        case, iv, mp, paths, ev, job = cases[name]
        assert rr.grid_entries(job, case.chroms, 10) == entries and rr.shift_of(job, case.chroms) == shift
        assert (entries <= rr.LOC_CAP) == (shift == 10)
    assert cases["wide4"][0].texts == cases["wide5"][0].texts
    text = cases["wide4"][0].texts["r"]
    digits = set(len(str(b[2] + 1)) for _, bl in rr.parse_mrf(text) for b in bl)
    assert {4, 9, 10} <= digits              # nine digits: the tile kernel's own; ten: handed to the list
    reg = cases["wide4"][5].regions("chrW0", 0)
    assert any(s == rr.WIDE_MID for s, _ in reg) and any(s == rr.WIDE_MID + 2048 for s, _ in reg) and any(s == rr.WIDE_MID - 2048 for s, _ in reg)


def test_limits_case_holds_the_first_and_last_bases(cases):
    case, iv, mp, paths, ev, job = cases["limits"]
    reads, _ = rr.route(job, case.texts["good"])
    ends, starts = set(r.blocks[-1][1] for r in reads.values()), set(r.blocks[0][0] for r in reads.values())
    assert rr.LIM - 1 in ends and -rr.LIM + 1 in starts and max(ends) == rr.LIM - 1 and min(starts) == -rr.LIM + 1
    totals = sorted(sum(e - s for s, e in r.blocks) for r in reads.values())
    assert totals[-2:] == [rr.BIG - 1, rr.BIG - 1] and sorted(len(r.blocks) for r in reads.values() if sum(e - s for s, e in r.blocks) == rr.BIG - 1) == [1, 3]
    for stem, n_blocks in (("big1", 1), ("big3", 3)):
        reads, _ = rr.route(job, case.texts[stem])
        big = [r for r in reads.values() if sum(e - s for s, e in r.blocks) == rr.BIG]
        assert len(big) == 1 and len(big[0].blocks) == n_blocks and len(reads) == 2
