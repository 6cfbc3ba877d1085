"""Wall-clock seconds of the differential splicing tests (lsq_as_*, test_as) on synthetic inputs of configs[4]'s shape:
200 k Fisher tables with Zipf-like depths up to 10^7, 400 k LRT, beta-binomial and Wilcoxon rows x 16 samples (8 + 8; the
beta-binomial test on the LRT's own rows).  Each entry
point returns after its results are on the host (it ends in a synchronise); a CLI run is test_as in-process, matrix
files in, output file out.  Prints one JSON line.

usage: python tools/as_bench.py [--repeat 3] [--seed 4]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lesseq_amd as L  # noqa: E402
from lesseq_amd import diffsplice as ds  # noqa: E402


def inputs(seed, n_tables=200000, n_rows=400000, n1=8, n2=8):
    rng = np.random.default_rng(seed)
    depth = np.minimum(1e7, 10.0 / rng.uniform(1e-7, 1, size=n_tables) ** 1.2).round()
    share = rng.uniform(0.05, 0.95, size=(n_tables, 4))
    cells = np.rint(depth[:, None] * share / share.sum(1, keepdims=True))
    total = np.exp(rng.uniform(np.log(5), np.log(1e5), size=(n_rows, n1 + n2))).round()
    count = rng.binomial(total.astype(np.int64), rng.uniform(0.1, 0.9, size=(n_rows, 1))).astype(np.float64)
    value = rng.beta(2, 2, size=(n_rows, n1 + n2))
    return cells, count, total, value


def best(f, repeat):
    t = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return min(t)


def write_matrix(path, values, prefix):
    with open(path, "w") as f:
        f.write("ID\t" + "\t".join("s%d" % j for j in range(values.shape[1])) + "\n")
        for i, r in enumerate(values):
            f.write("%s%d\t%s\n" % (prefix, i, "\t".join(repr(float(v)) for v in r)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--no-cli", action="store_true")
    a = ap.parse_args()
    cells, count, total, value = inputs(a.seed)
    ctx = L.Context(int(os.environ.get("LSQ_DEVICE", "0")))
    ds.fisher(ctx, cells[:1000])                 # first launches: code objects loaded
    p_f = ds.fisher(ctx, cells)
    _, p_l = ds.lrt(ctx, count, total, 8, 8)
    _, p_w = ds.wilcox(ctx, value, 8, 8)
    p_b = ds.betabin(ctx, count, total, 8, 8)[4]
    res = {"tables": len(cells), "rows": len(count), "samples": 16}
    res["fisher_s"] = best(lambda: ds.fisher(ctx, cells), a.repeat)
    res["lrt_s"] = best(lambda: ds.lrt(ctx, count, total, 8, 8), a.repeat)
    res["betabin_s"] = best(lambda: ds.betabin(ctx, count, total, 8, 8), a.repeat)
    res["wilcox_s"] = best(lambda: ds.wilcox(ctx, value, 8, 8), a.repeat)
    res["adjust_200k_s"] = best(lambda: ds.adjust(ctx, p_f), a.repeat)
    res["adjust_400k_s"] = best(lambda: ds.adjust(ctx, p_l), a.repeat)
    res["na_p"] = {"fisher": int(np.isnan(p_f).sum()), "lrt": int(np.isnan(p_l).sum()), "betabin": int(np.isnan(p_b).sum()), "wilcox": int(np.isnan(p_w).sum())}
    if not a.no_cli:
        with tempfile.TemporaryDirectory() as d:
            fm, one, al, rel, out = (os.path.join(d, n) for n in ("fisher.txt", "one.txt", "all.txt", "rel.txt", "out.txt"))
            write_matrix(fm, cells.reshape(-1, 2), "f")
            write_matrix(one, count, "r")
            write_matrix(al, total, "r")
            write_matrix(rel, value, "r")
            runs = {"cli_fisher_s": ["fisher", fm, out], "cli_lrt_s": ["lrt", one, al, "8", "8", out],
                    "cli_betabin_s": ["betabin", one, al, "8", "8", out], "cli_wilcox_s": ["wilcox", rel, "8", "8", out]}
            for k, argv in runs.items():
                def run():
                    rc, _ = L.cli_run("test_as", argv)
                    assert rc == 0, (k, rc)
                res[k] = best(run, a.repeat)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
