"""The inputs the cluster tests share (tests/test_clusters_host.py, tests/test_clusters_gpu.py): one annotation, the cases as
samples of (chromosome index, start, end, reads) rows with their thresholds, and the comparison of a table with the reference."""
import random

import lesseq_amd as L
import junction_ref as J
import clusters_ref as R

# The dictionary is the annotation's order -- chr2 (0), chr10 (1), chr1 (2) --, the table's order is chr1, chr10, chr2
CHR2, CHR10, CHR1 = 0, 1, 2
NAMES = ["chr2", "chr10", "chr1"]
SORT_TILE = L.junctions.SORT_TILE


def annotation_lines():
    return [J.interval_line("a.1", "chr2", "+", [(50, 100), (900, 1000)]),
            J.interval_line("b.1", "chr10", "+", [(100, 200), (400, 450)]),
            J.interval_line("b.2", "chr10", "-", [(2900, 3000), (4000, 4100)]),
            J.interval_line("c.1", "chr1", "-", [(10, 20), (30, 40)])]


def write_annotation(d):
    """(interval text, paths) of the cases' annotation, written into d"""
    interval, _, paths = J.write_case(d, "clusters", annotation_lines(), [])
    return interval, paths


def worked_example():
    both = [(CHR10, 200, 400), (CHR10, 200, 500), (CHR10, 300, 900), (CHR10, 1000, 2000), (CHR10, 3000, 200000), (CHR10, 3000, 4000), (CHR10, 3500, 4000), (CHR2, 100, 900)]
    s1 = [(CHR10, 100, 900, 5)] + [j + (r,) for j, r in zip(both, (3, 1, 2, 40, 9, 10, 10, 50))]
    s2 = [j + (r,) for j, r in zip(both, (4, 1, 2, 40, 9, 10, 10, 50))]
    return [s1, s2], dict(min_cluster_reads=5)


def staircase(n, broken=False):
    """n rows that alternately share a start and an end: one chain; broken: the middle row made long, which cuts the chain"""
    rows = []
    for i in range(n):
        m = i // 2
        rows.append((CHR1, 1000 + m, 1000000 + m + i % 2, 1))
    if broken:
        c, s, e, r = rows[n // 2]
        rows[n // 2] = (c, s, e + 10000000, r)
    return [rows], dict(max_intron=2000000, min_cluster_reads=1)


def pairs(n_rows):
    """n_rows pooled rows, clusters of two rows each (an odd last row is a singleton): links across every edge of a tile"""
    rows = [(CHR10, 1000 + 200 * (i // 2), 1000 + 200 * (i // 2) + (50 if i % 2 == 0 else 80), 1 + i % 3) for i in range(n_rows)]
    return [rows], dict(min_cluster_reads=3)


def random_pool(seed=20, n_introns=5000, n_samples=4):
    """n_introns distinct introns on three chromosomes, their ends drawn from so few sites that components of many sizes arise"""
    rng = random.Random(seed)
    sites = {c: sorted(rng.sample(range(1000, 400000), 1500)) for c in range(3)}
    introns = set()
    while len(introns) < n_introns:
        c = rng.randrange(3)
        a, b = sorted(rng.sample(sites[c], 2))
        introns.add((c, a, b))
    introns = sorted(introns)
    samples = []
    for _ in range(n_samples):
        rows = [j + (rng.choice((1, 1, 2, 5, 30)),) for j in introns if rng.random() < 0.6]
        rng.shuffle(rows)
        samples.append(rows)
    return samples, dict(min_reads=3, max_intron=150000, min_cluster_reads=30)


def small_cases():
    """{name: (samples, thresholds)}: the cases of a handful of rows"""
    bridge = [[(CHR1, 100, 200, 10), (CHR1, 100, 250, 10), (CHR1, 400, 500, 10), (CHR1, 450, 500, 10), (CHR1, 100, 500, 1)]]
    three = [[(CHR1, 100, 200, 1), (CHR1, 100, 300, 1), (CHR1, 150, 200, 5)], [(CHR1, 100, 200, 1), (CHR1, 100, 300, 1)], [(CHR1, 100, 200, 1)]]
    lengths = [[(CHR2, 100, 1100, 4), (CHR2, 100, 1101, 4), (CHR2, 50, 1100, 4), (CHR2, 100, 500000, 4)]]
    totals = [[(CHR1, 100, 200, 10), (CHR1, 100, 300, 5)], [(CHR1, 100, 200, 15), (CHR1, 1000, 1200, 14), (CHR1, 1100, 1200, 15)]]
    return {
        "worked_example": worked_example(),
        "shared_start_only": ([[(CHR1, 100, 200, 20), (CHR1, 100, 300, 20), (CHR1, 400, 500, 20)]], dict(min_cluster_reads=1)),
        "shared_end_only": ([[(CHR1, 100, 300, 20), (CHR1, 200, 300, 20), (CHR1, 400, 500, 20)]], dict(min_cluster_reads=1)),
        "start_equals_end": ([[(CHR1, 100, 200, 20), (CHR1, 200, 300, 20)]], dict(min_cluster_reads=1)),
        "two_chromosomes": ([[(CHR1, 100, 200, 20), (CHR10, 100, 200, 20), (CHR2, 100, 200, 20), (CHR2, 100, 300, 20)]], dict(min_cluster_reads=1)),
        "bridge_kept": (bridge, dict(min_reads=1, min_cluster_reads=1)),
        "bridge_weak": (bridge, dict(min_reads=2, min_cluster_reads=1)),
        "three_samples": (three, dict(min_reads=3, min_cluster_reads=1)),
        "max_intron_zero": (lengths, dict(max_intron=0, min_cluster_reads=1)),
        "length_exactly_l": (lengths, dict(max_intron=1000, min_cluster_reads=1)),
        "long_and_weak": (lengths, dict(min_reads=5, max_intron=1000, min_cluster_reads=1)),
        "cluster_total": (totals, dict(min_cluster_reads=30)),
        "duplicate_rows": ([[(CHR1, 100, 200, 3), (CHR1, 100, 300, 4), (CHR1, 100, 200, 5), (CHR1, 100, 200, 0)], [(CHR1, 100, 300, 2), (CHR1, 100, 300, 2)]], dict(min_cluster_reads=1)),
        "empty_sample": ([[(CHR1, 100, 200, 20), (CHR1, 100, 300, 20)], [], [(CHR1, 100, 200, 20)]], dict(min_cluster_reads=1)),
        "zero_reads": ([[(CHR1, 100, 200, 0), (CHR1, 100, 300, 20), (CHR1, 150, 300, 20)]], dict(min_cluster_reads=1)),
        "empty_pool": ([], dict()),
        "samples_without_rows": ([[], []], dict()),
    }


def large_cases():
    """{name: (samples, thresholds)}: the chain, the sizes around a tile of the sort and a block of the scan, the random pool"""
    cases = {"staircase": staircase((1 << 15) + 1), "staircase_broken": staircase((1 << 15) + 1, broken=True), "random": random_pool()}
    for n in (SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, 3 * SORT_TILE + 1):
        cases["pairs_%d" % n] = pairs(n)
    return cases


def pool_of(index, samples):
    pool = L.ClusterPool(index)
    for rows in samples:
        pool.add_rows([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows])
    return pool


def reference(interval, samples, opts):
    return R.solve(NAMES, samples, ann=J.introns(interval), **opts)


def same(got, want):
    """a library table against the reference's result: arrays, count matrix, report and both texts"""
    assert got.rows() == want.rows
    assert got.counts.tolist() == want.counts
    assert got.report == want.report
    assert got.text() == want.text
    assert [got.sample_text(k) for k in range(got.n_samples)] == want.sample_texts


def same_tables(a, b):
    """two library tables: every array, the report and the texts"""
    for k in ("chrom", "start", "end", "ann", "reads", "samples", "cluster", "status", "counts"):
        assert (getattr(a, k) == getattr(b, k)).all(), k
    assert a.report == b.report and a.text() == b.text() and a.n_samples == b.n_samples
    assert [a.sample_text(k) for k in range(a.n_samples)] == [b.sample_text(k) for k in range(b.n_samples)]
