"""lsq_fim_kernel (lsq_em.hip) and the host code behind it (lsq_annot.cpp fim_start_classes) tested directly: the direct
set of tests/fim_ref.py -- structures and class counts chosen by hand, no read involved -- goes in through
lsq_results_set_counts, and the matrices and the two variance estimates that lsq_results_fim returns are held against
the exact rational reference evaluated AT THE THETA THE DEVICE RETURNED, within the bounds derived in fim_ref.py.
Need an MI355X: python -m pytest tests -m gpu."""
import math

import numpy as np
import pytest

import lesseq_amd as L
import fim_ref as F
from golden_inputs import mrf_line, transcript_blocks
from test_em_direct_gpu import context, counts_array, solution
from test_fim_reference_host import direct_events

pytestmark = pytest.mark.gpu

M = len(F.READ_FILES)


def matrices(ev, fim_out):
    """fim() -> [event][read file] = (D x D array, by_diag, by_inv), after the layout has been checked"""
    off, f, vd, vi = fim_out
    assert f.shape == (M, int(off[-1])) and vd.shape == vi.shape == (M, len(ev))
    out = []
    for e in range(len(ev)):
        D = ev.K(e) - 1
        assert int(off[e + 1]) - int(off[e]) == D * D, (e, off[e], off[e + 1])
        out.append([(f[m, int(off[e]):int(off[e + 1])].reshape(D, D).copy(), float(vd[m, e]), float(vi[m, e])) for m in range(M)])
    return out


def thetas_of(ev, theta):
    out, io = [], 0
    for e in range(len(ev)):
        out.append([float(x) for x in theta[io:io + ev.K(e)]])
        io += ev.K(e)
    return out


def ratios(cases, refs, got):
    """the error / bound ratios of every (event, read file): three lists of (ratio, what) -- matrix entries, by_diag, by_inv --
    and the by_inv values of the exactly singular matrices"""
    mat, diag, inv, singular = [], [], [], []
    for c, r, g in zip(cases, refs, got):
        for m in range(M):
            f, (I, by_diag, by_inv) = r[m], g[m]
            what = "%s, read file %d" % (c.name, m)
            for p in range(f.D):
                for q in range(f.D):
                    mat.append((F.error_ratio(float(I[p, q]), f.I[p][q], f.matrix_bound(p, q)), "%s, entry (%d, %d): %r against %r" % (what, p, q, I[p, q], float(f.I[p][q]))))
            if f.by_diag == F.INF:
                diag.append((0.0 if by_diag == F.INF else F.INF, "%s: by_diag %r, the reference inf" % (what, by_diag)))
            else:
                diag.append((F.error_ratio(by_diag, f.by_diag, f.by_diag_rel_bound() * f.by_diag), "%s: by_diag %r against %r" % (what, by_diag, float(f.by_diag))))
            if f.det != 0:
                inv.append((F.error_ratio(by_inv, f.by_inv, f.by_inv_bound()), "%s: by_inv %r against %r (kappa %.3g)" % (what, by_inv, float(f.by_inv), float(f.kappa))))
            else:
                singular.append((by_inv, what))
    return mat, diag, inv, singular


def worst(rs):
    return max(rs, key=lambda x: x[0])


@pytest.fixture(scope="module")
def direct(tmp_path_factory):
    d = tmp_path_factory.mktemp("fim")
    cases = F.direct_set()
    ev = direct_events(d)
    cnt, bases = counts_array(ev, [c.counts for c in cases])
    ctx = context(ev)
    order = ctx.device_order().tolist()
    ctx.set_counts(cnt, bases)
    ctx.solve()
    first = ctx.fim()
    first = tuple(x.copy() for x in first)
    sol = solution(ctx)
    again = tuple(x.copy() for x in ctx.fim())
    thetas = thetas_of(ev, sol[0])
    assert np.isfinite(sol[0]).all() and (sol[0] >= 0).all()
    refs = [[F.reference_at(c, m, th) for m in range(M)] for c, th in zip(cases, thetas)]
    got = matrices(ev, first)
    r = ratios(cases, refs, got)
    print("\nfim direct set, %d events x %d read files: largest error / bound -- matrix %.3g, by_diag %.3g, by_inv %.3g"
          % (len(cases), M, worst(r[0])[0], worst(r[1])[0], worst(r[2])[0]))
    yield dict(d=d, ev=ev, cases=cases, cnt=cnt, bases=bases, ctx=ctx, order=order, sol=sol, thetas=thetas, refs=refs, first=first, again=again,
               got=got, ratios=r)
    ctx.close()


def test_the_set_hides_nothing(direct):
    """no event flagged, every theta a number; every K, both read files, every geometry edge and every count pattern among
    the checked cases, two thirds of the regular ones with a by_inv bound below 1e-9 relative -- at the device's theta; events
    of unequal K are neighbours in output order and the device's order is another one"""
    cases, sol = direct["cases"], direct["sol"]
    assert (sol[3] == 0).all(), [cases[e].name for e in np.flatnonzero(sol[3])]
    got = F.coverage(cases, direct["thetas"], direct["refs"])
    print(got)
    order = direct["order"]
    assert sorted(order) == list(range(len(cases))) and order != list(range(len(cases)))
    assert any(cases[a].K != cases[b].K for a, b in zip(order, order[1:]))
    assert len(direct["ratios"][0]) == M * sum((c.K - 1) ** 2 for c in cases)
    assert len(direct["ratios"][1]) == M * len(cases) and len(direct["ratios"][2]) == got["regular"] + M * sum(c.K == 1 for c in cases)


def test_matrix_entries_within_the_bound(direct):
    bad = [w for r, w in direct["ratios"][0] if not r <= 1]
    print("matrix: largest error / bound %.3g (%s)" % worst(direct["ratios"][0]))
    assert not bad, "%d entries beyond C1 eps A_pq:\n  %s" % (len(bad), "\n  ".join(bad[:12]))


def test_variance_by_the_diagonal_within_the_bound(direct):
    bad = [w for r, w in direct["ratios"][1] if not r <= 1]
    print("by_diag: largest error / bound %.3g (%s)" % worst(direct["ratios"][1]))
    assert not bad, "%d values beyond (C1 + D + 2) eps relative:\n  %s" % (len(bad), "\n  ".join(bad[:12]))
    assert sum(1 for c, r in zip(direct["cases"], direct["refs"]) for m in range(M) if c.K > 1 and r[m].by_diag == F.INF) >= 1


def test_variance_by_the_inverse_within_the_bound(direct):
    bad = [w for r, w in direct["ratios"][2] if not r <= 1]
    print("by_inv: largest error / bound %.3g (%s)" % worst(direct["ratios"][2]))
    assert not bad, "%d values beyond (C1 + 3 D^3 2^(D-1)) eps kappa S:\n  %s" % (len(bad), "\n  ".join(bad[:12]))


def test_variance_by_the_inverse_of_a_singular_matrix(direct):
    """det = 0 exactly: what the LU makes of it is no number, or at least 1e11 in magnitude"""
    singular = direct["ratios"][3]
    assert len(singular) >= 4
    for v, what in singular:
        print("singular: %s: by_inv %r" % (what, v))
    bad = [(what, v) for v, what in singular if math.isfinite(v) and abs(v) < 1e11]
    assert not bad, bad


def test_one_isoform(direct):
    ev, (off, f, vd, vi) = direct["ev"], direct["first"]
    ones = [e for e, c in enumerate(direct["cases"]) if c.K == 1]
    assert len(ones) >= 3
    for e in ones:
        assert off[e] == off[e + 1]
        assert (vd[:, e] == 0).all() and (vi[:, e] == 0).all()


def test_layout_and_a_second_solve(direct):
    """fim_offsets is (K - 1)^2 in output order and lsq_results_fim_size its end; fim() twice gives the same bits; after a
    solve on other counts it gives the matrices of THAT theta, and back on the first counts the first bits again"""
    ev, cases, ctx = direct["ev"], direct["cases"], direct["ctx"]
    off = direct["first"][0]
    assert off.tolist() == np.concatenate([[0], np.cumsum([(c.K - 1) ** 2 for c in cases])]).tolist()
    assert L.lib.lsq_results_fim_size(ctx.h) == int(off[-1])
    for a, b in zip(direct["first"], direct["again"]):
        assert np.array_equal(a, b, equal_nan=True)
    other = direct["cnt"] * (np.uint64(1) + (np.arange(direct["cnt"].shape[1], dtype=np.uint64) % np.uint64(3))[None, :])
    ctx.set_counts(other, other)
    ctx.solve()
    second = tuple(x.copy() for x in ctx.fim())
    sol = solution(ctx)
    thetas = thetas_of(ev, sol[0])
    assert np.isfinite(sol[0]).all() and sum(a != b for a, b in zip(thetas, direct["thetas"])) > len(cases) // 2
    refs = [[F.reference_at(c, m, th) for m in range(M)] for c, th in zip(cases, thetas)]
    r = ratios(cases, refs, matrices(ev, second))
    for k, name in enumerate(("matrix", "by_diag", "by_inv")):
        bad = [w for x, w in r[k] if not x <= 1]
        assert not bad, "second solve, %s: %s" % (name, "\n  ".join(bad[:12]))
    ctx.set_counts(direct["cnt"], direct["bases"])
    ctx.solve()
    third = ctx.fim()
    for a, b in zip(direct["first"], third):
        assert np.array_equal(a, b, equal_nan=True)


def test_fim_lines_carry_what_lsq_results_fim_returns(direct, monkeypatch):
    """`solve ... --fim` in this process on reads laid over three events of the set: every number of a `#fim` line is, digit
    for digit (%.17g), the one lsq_results_fim returns for the same reads"""
    ev, cases, d = direct["ev"], direct["cases"], direct["d"]
    chosen = [next(e for e, c in enumerate(cases) if c.K == K and c.pattern == "balanced" and min(min(a) for a in c.ars) > 1) for K in (2, 4, 6)]
    paths = []
    for m, (rt, R) in enumerate(F.READ_FILES):
        lines = ["AlignmentBlocks\n"]
        for e in chosen:
            segs = ev.segments(e)
            for j in range(ev.K(e)):
                form = [segs[n] for n in cases[e].isoforms[j]]
                n_starts = sum(b - a for a, b in form) - R + 1
                for t in range(0, n_starts, max(n_starts // (4 + j), 1)):
                    lines.append(mrf_line("chr1", "+", transcript_blocks(form, t, R)))
        paths.append(str(d / ("reads%d.mrf" % m)))
        with open(paths[-1], "w") as f:
            f.write("".join(lines))
    ctx = context(ev)
    for m in range(M):
        ctx.upload_reads(m, L.Reads.from_mrf(paths[m], ev))
    ctx.count()
    ctx.solve()
    theta, _, _, flags = solution(ctx)
    off, f, vd, vi = ctx.fim()
    ctx.close()
    assert (flags == 0).all()
    thetas = thetas_of(ev, theta)
    for e in chosen:
        assert len(set(thetas[e])) > 1, (cases[e].name, thetas[e])           # the reads moved theta off 1 / K
    monkeypatch.chdir(d)
    argv = ["0", "fim", "./", "LH_GENE_TXT", "fim.interval", "UCSC_GENE2ISOFORM", "fim.map", "0", str(len(ev))]
    for m, (rt, R) in enumerate(F.READ_FILES):
        n_reads = len(open(paths[m]).read().splitlines()) - 1
        argv += ["MRF_SINGLE", rt, str(R), "reads%d.mrf" % m, str(n_reads * R)]
    rc0, plain = L.cli_run("solve", argv)
    rc1, with_fim = L.cli_run("solve", argv + ["--fim"])
    assert rc0 == rc1 == 0 and with_fim.startswith(plain)
    extra = with_fim[len(plain):].split("\n")[:-1]
    assert len(extra) == len(ev) * M and all(x.startswith("#fim\t") for x in extra)
    index = {c.name: e for e, c in enumerate(cases)}
    seen = set()
    for line in extra:
        t = line.split("\t")
        e, m = index[t[1]], int(t[2])
        D = cases[e].K - 1
        vals = [float(x) for x in t[3:]]
        assert len(vals) == 2 + D * D, line
        want = [vd[m, e], vi[m, e]] + f[m, int(off[e]):int(off[e + 1])].tolist()
        assert all(a == b or (a != a and b != b) for a, b in zip(vals, want)), (line, want)
        seen.add((e, m))
    assert all((e, m) in seen for e in chosen for m in range(M))
