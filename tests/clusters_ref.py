"""Intron clusters of several samples: the definition (include/lesseq_hip.h, lsq_cl_*) in plain Python -- a dict of
pooled rows, the two row filters, a breadth-first walk over shared (chromosome, start) and shared (chromosome, end).  Written from
the definition; it shares nothing with the library."""
from collections import deque

REPORT = ("samples", "pooled_rows", "introns", "long_rows", "weak_rows", "kept_rows", "components", "singletons", "weak_clusters", "clusters", "printed_rows")
PRINTED, WEAK_ROW, LONG_ROW, SINGLETON, WEAK_CLUSTER = range(5)


class Result:
    """rows: [(chromosome name, start, end, ann, reads, samples, cluster, status)] in table order; counts: per row the reads per
    sample; report; text; sample_texts"""


def solve(names, samples, min_reads=1, max_intron=100000, min_cluster_reads=30, ann=None):
    """names: the chromosome dictionary (an index is a place in it); samples: per sample [(chromosome index, start, end, reads)];
    ann: {(chromosome name, start, end): character} of the annotation's introns"""
    ann = ann or {}
    n_samples = len(samples)
    pooled = {}
    for k, rows in enumerate(samples):
        for c, s, e, r in rows:
            assert 0 <= c < len(names) and s < e
            pooled.setdefault((names[c], s, e), [0] * n_samples)[k] += r
    order = sorted(pooled, key=lambda j: (j[0].encode(), j[1], j[2]))       # chromosome name bytewise, start, end
    status = {}
    for j in order:
        reads = sum(pooled[j])
        if max_intron != 0 and j[2] - j[1] > max_intron:
            status[j] = LONG_ROW
        elif reads < min_reads:
            status[j] = WEAK_ROW
    kept = [j for j in order if j not in status]
    by_start, by_end = {}, {}
    for j in kept:
        by_start.setdefault((j[0], j[1]), []).append(j)
        by_end.setdefault((j[0], j[2]), []).append(j)
    component = {}
    components = []
    for j in kept:                                                          # in table order: a component is found at its first row
        if j in component:
            continue
        members, queue = [], deque([j])
        component[j] = len(components)
        while queue:
            x = queue.popleft()
            members.append(x)
            for y in by_start[(x[0], x[1])] + by_end[(x[0], x[2])]:
                if y not in component:
                    component[y] = len(components)
                    queue.append(y)
        components.append(members)
    number = {}
    n_single = n_weak_clusters = 0
    for q, members in enumerate(components):
        if len(members) == 1:
            n_single += 1
            status[members[0]] = SINGLETON
        elif sum(sum(pooled[j]) for j in members) < min_cluster_reads:
            n_weak_clusters += 1
            for j in members:
                status[j] = WEAK_CLUSTER
        else:
            number[q] = len(number) + 1
            for j in members:
                status[j] = PRINTED
    out = Result()
    out.rows = [(j[0], j[1], j[2], ann.get(j, "."), sum(pooled[j]), sum(1 for v in pooled[j] if v > 0), number[component[j]] if status[j] == PRINTED else 0, status[j])
                for j in order]
    out.counts = [list(pooled[j]) for j in order]
    printed = sorted((j for j in order if status[j] == PRINTED), key=lambda j: number[component[j]])       # stable: table order inside a cluster
    n_status = [sum(1 for j in order if status[j] == s) for s in range(5)]
    out.report = dict(zip(REPORT, (n_samples, sum(len(rows) for rows in samples), len(order), n_status[LONG_ROW], n_status[WEAK_ROW], len(kept), len(components),
                                   n_single, n_weak_clusters, len(number), len(printed))))
    out.text = "".join("clu_%d\t%s\t%d\t%d\t%s\t%d\t%d\n" % (number[component[j]], j[0], j[1] + 1, j[2], ann.get(j, "."), sum(pooled[j]), sum(1 for v in pooled[j] if v > 0))
                       for j in printed)
    out.sample_texts = []
    for k in range(n_samples):
        total = {q: sum(pooled[j][k] for j in members) for q, members in enumerate(components)}
        out.sample_texts.append("".join("clu_%d\t%d\t%s:%d:%d\t%d\n" % (number[component[j]], total[component[j]], j[0], j[1] + 1, j[2], pooled[j][k]) for j in printed))
    return out
