"""The shortcut table of a packed bucket (csrc/lsq_internal.hpp, built in csrc/lsq_annot.cpp plan_device) against a plain
model over every base of the bucket (count_cells_ref.cells): the cells the count kernel's streaming loops settle reads by.
The records come out of the compiled image through lsq_debug_bucket_cells; no device."""
import pytest

import lesseq_amd as L
import count_cells_ref as cr
import count_paths_inputs as ci

NE = cr.CELL_NO_END
EMPTY, SHARED = cr.CELL_INFO_EMPTY, cr.CELL_INFO_SHARED
BOTH, NEAR, FAR = cr.CELLX_BOTH, cr.CELLX_NEAR_NO_ABUT, cr.CELLX_FAR_NO_ABUT

# The cells of the events A, B, C, worked out by hand.  Bucket order: A (span 1000..1500) = 0, C (1450..2130) = 1, B (2000..2700) = 2.
# info of a one-owner cell: event << 8 | segment << 2 | "lo is the segment's start"; of a start cell: event << 8 | 63 << 2.
ABC_CELLS = [
    (1000, 1001, 1001, 1499, 0 << 8 | 63 << 2, 0),          # A's first base: A's first segment alone covers it -- a start cell up to gene_end - 1
    (1001, 1100, 1100, 1160, 0 << 8 | 0 << 2, 0),           # A0; A1 abuts it: e2 = A1's end
    (1100, 1160, 1160, 1160, 0 << 8 | 1 << 2 | 1, 0),       # A1
    (1160, 1400, NE, NE, EMPTY, 0),                         # A's intron
    (1400, 1450, 1500, 1500, 0 << 8 | 2 << 2 | 1, 0),       # A2 before C starts
    # [1450, 1451): C's first base, inside A2 too -- no cell
    (1451, 1500, 1500, 1520, SHARED, BOTH | NEAR | 1),      # A2 (ends first; nothing abuts it) and C0 (C1 abuts it): far owner C = 1
    (1500, 1520, 1520, 1600, 1 << 8 | 0 << 2, 0),           # C0 behind A2; C1 abuts it
    (1520, 1600, 1600, 1600, 1 << 8 | 1 << 2 | 1, 0),       # C1
    (1600, 2000, NE, NE, EMPTY, 0),
    (2000, 2001, 2001, 2699, 2 << 8 | 63 << 2, 0),          # B's first base: a start cell
    (2001, 2050, 2100, 2100, 2 << 8 | 0 << 2, 0),           # B0 before C2 starts
    (2050, 2100, 2100, 2130, SHARED, BOTH | NEAR | FAR | 1),   # B0 (ends first) and C2: nothing abuts either
    (2100, 2130, 2130, 2130, 1 << 8 | 2 << 2, 0),           # C2 behind B0
    (2130, 2300, NE, NE, EMPTY, 0),
    (2300, 2360, 2360, 2360, 2 << 8 | 1 << 2 | 1, 0),       # B1
    (2360, 2600, NE, NE, EMPTY, 0),
    (2600, 2700, 2700, 2700, 2 << 8 | 2 << 2 | 1, 0),       # B2
]


def compiled(tmp_path, genes, R=100):
    iv, mp = ci.write_annotation(str(tmp_path), "g", genes)
    return L.Events(L.Annotation(iv, mp), ("SHORT_READ",), (R,))


def test_hand_worked_cells_of_the_threshold_events(tmp_path):
    """A, B, C of test_reads_on_every_threshold_of_the_streaming_loops_vs_oracle: the library's cells, the model's and a list
    worked out by hand are one and the same"""
    ev = compiled(tmp_path, ci.ABC)
    assert ev.num_buckets == 1
    (b, M, idx), = ci.models_of(ev)
    assert [e.name for e in M.events] == ["A", "C", "B"]
    assert {e.name: e.segs for e in M.events} == ci.ABC_SEGS
    assert [cr.encode(c) for c in M.cells] == ABC_CELLS
    assert ev.bucket_cells(b) == ABC_CELLS


def test_cells_with_three_owners_and_a_first_base_inside_another_segment(tmp_path):
    """with D (the bases [1471, 1490) lie in segments of A, C and D: no cell; D's first base in two other segments: none either)
    and E (its first base lies inside A's first segment: no start cell; two-owner cells whose nearer owner has an abutting
    segment; a one-owner cell of E behind A's second segment)"""
    ev = compiled(tmp_path, ci.ABC + ci.DE)
    assert ev.num_buckets == 1
    (b, M, idx), = ci.models_of(ev)
    segs = dict(ci.ABC_SEGS, **ci.DE_SEGS)
    assert {e.name: e.segs for e in M.events} == segs
    assert [e.name for e in M.events] == ["A", "E", "C", "D", "B"]
    got = ev.bucket_cells(b)
    assert got == [cr.encode(c) for c in M.cells]
    at = {c[0]: c for c in got}
    # hand-worked, where D and E change the table
    assert 1040 not in at and 1470 not in at and 1471 not in at              # first bases under other segments; three owners
    assert at[1041] == (1041, 1100, 1100, 1180, SHARED, BOTH | FAR | 1)      # A0 (A1 abuts it) and E0 (nothing abuts): far owner E = 1
    assert at[1100] == (1100, 1160, 1160, 1180, SHARED, BOTH | NEAR | FAR | 1)
    assert at[1160] == (1160, 1180, 1180, 1180, 1 << 8 | 0 << 2, 0)         # E0 alone
    assert at[1451] == (1451, 1470, 1500, 1520, SHARED, BOTH | NEAR | 2)     # A2 and C0 up to D's first base; C = 2 now
    assert at[1490] == (1490, 1500, 1500, 1520, SHARED, BOTH | NEAR | 2)
    assert at[2100] == (2100, 2110, 2130, 2130, 2 << 8 | 2 << 2, 0)         # C2 between B0's end and D1's start
    assert at[2110] == (2110, 2130, 2130, 2160, SHARED, BOTH | NEAR | 3)     # C2 (nothing abuts it) and D1 (D2 abuts it): far owner D = 3
    assert at[2130] == (2130, 2160, 2160, 2200, 3 << 8 | 1 << 2, 0)         # D1 behind C2; D2 abuts it
    assert at[1200] == (1200, 1225, 1225, 1250, 1 << 8 | 1 << 2 | 1, 0)     # E1; E2 abuts it


@pytest.mark.parametrize("seed", list(range(1, 25)))
def test_cells_of_seeded_small_gene_sets(seed, tmp_path):
    ev = compiled(tmp_path, ci.seeded_genes(seed))
    n_cells = 0
    for b, M, idx in ci.models_of(ev):
        want = [cr.encode(c) for c in M.cells]
        got = ev.bucket_cells(b)
        twins = {c["lo"] for c in M.cells if c.get("twin")}
        # (twins -- two owners with one and the same interval: which of them the library calls the nearer is open (std::sort);
        # the cell, its thresholds and its being shared still hold)
        norm = lambda c: c if c[0] not in twins else c[:5] + (c[5] & BOTH,)
        assert [norm(c) for c in got] == [norm(c) for c in want], (seed, b)
        n_cells += len(got)
    assert n_cells > 0, "no packed bucket: the set tests nothing"


def test_the_seeded_sets_reach_every_kind_of_cell(tmp_path):
    """... start cells, empty, one owner with and without an abutting segment, two owners with each pair of no-abut flags, stretches
    of three owners, and first bases that are no cell"""
    seen = set()
    for seed in range(1, 25):
        ev = compiled(tmp_path, ci.seeded_genes(seed))
        for b, M, idx in ci.models_of(ev):
            for c in M.cells:
                seen.add(c["kind"] if c["kind"] != "two" else ("two", c["near_free"], c["far_free"]))
                if c["kind"] == "one":
                    seen.add(("one", c["e2"] > c["e1"]))
            covered_by_cells = {p for c in M.cells for p in range(c["lo"], c["hi"])}
            for e in M.events:
                if e.gs not in covered_by_cells:
                    seen.add("first base without a cell")
            for p in range(min(e.gs for e in M.events), max(e.ge for e in M.events)):
                if p not in covered_by_cells and sum(1 for e in M.events for s, t in e.segs if s <= p < t) >= 3:
                    seen.add("three owners")
    want = {"start", "empty", "one", ("one", True), ("one", False), ("two", True, True), ("two", True, False), ("two", False, True),
            ("two", False, False), "first base without a cell", "three owners"}
    assert want <= seen, want - seen


def test_bad_arguments_and_buckets_without_cells(tmp_path, monkeypatch):
    ev = compiled(tmp_path, ci.ABC)
    with pytest.raises(ValueError):
        ev.bucket_cells(1)
    with pytest.raises(ValueError):
        ev.bucket_events(-1)
    assert L.lib.lsq_debug_bucket_cells(ev.h, 0, None, None, None, None, None, None, 4) == -1
    monkeypatch.setenv("LSQ_FORCE_GENERIC", "1")          # generic records: no cells
    ev = compiled(tmp_path, ci.ABC)
    assert ev.bucket_events(0)[0] == 0 and ev.bucket_cells(0) == []


@pytest.mark.parametrize("kernel", cr.KERNELS)
def test_every_case_file_holds_its_thresholds_and_equalities(kernel, tmp_path):
    """the files tests/test_count_paths_gpu.py runs, made here without a device: every verdict of the kernel has at least 300
    reads, each with that verdict in the model, and among them the reads on and beside the threshold that governs the verdict
    and -- where the 98 % rule decides -- on equality and beside it (count_paths_inputs.required_tags): thinning the candidates
    to a file's size must never lose those.  E.g. `gone`: 50 x (end - e2) == length and one base more; one base less is
    park_past's."""
    ev = compiled(tmp_path, ci.ABC + ci.DE)
    (b, M, idx), = ci.models_of(ev)
    cases = ci.case_files(M, ev.covered(ci.CHROM))
    req = ci.required_tags(kernel)
    assert set(req) == set(ci.verdict_names(kernel))
    for v in ci.verdict_names(kernel):
        reads = cases.get((v, kernel), [])
        assert len(reads) >= 300, (kernel, v, len(reads))
        have = {}
        for rd in reads:
            got = cr.verdict1(M, rd, kernel)[0] if len(rd) == 2 else cr.verdict2(M, rd, kernel, "lead")[0]
            assert got == ("J" if v == "same" else v), (kernel, v, rd, got)
            for name, off in ci.tags(M, rd):
                have.setdefault(name, set()).add(off)
        for name, offs in req[v].items():
            assert offs <= have.get(name, set()), (kernel, v, name, "wanted", sorted(offs), "held", sorted(have.get(name, set())))
    if kernel != "wide":
        # the read the 98 % rule puts exactly on equality behind the farther owner's free end, by hand: cell [2050, 2100) of B0
        # and C2, C2 ends at 2130 and nothing abuts it; [2081, 2131) has 50 bases and overhangs by one: 50 x 1 == 50
        assert (2081, 2131) in cases[("gone", kernel)] and (2082, 2131) in cases[("gone", kernel)]
        assert (2080, 2131) in cases[("park_past", kernel)]
