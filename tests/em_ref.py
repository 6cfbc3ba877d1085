"""The reference of the direct EM tests: the EM of common/read.h:592-660 on compatibility-class counts, in Python's
decimal at 40 digits, with the whole trajectory kept; a plain float64 restatement that only sets a tolerance; the rule
by which a kernel's result is accepted against a trajectory; and the case sets of tests/test_em_reference_host.py and
tests/test_em_direct_gpu.py.  No GPU, no library call: pure Python.

An event has K isoforms and 2^K - 1 compatibility classes (class c = 1 .. 2^K - 1: bit j set = compatible with isoform
j).  counts[m][c - 1] reads of read file m fall into class c; G[m][j] = 1 / ARS of isoform j for read file m (0 for ARS
0).  Start 1/K; step theta_j = z_j / n with z_j = sum over (m, c) of counts * theta_j G_j / s, s = sum over the class's
isoforms of theta_j G_j; log-likelihood sum of counts * log s; test value |1 - ll_old / ll_new|, the loop goes on
while it is > 1e-6.

Degenerate rows as oracle/lsq_oracle.c and IEEE arithmetic settle them (lsq_em.hip em_crit: "-inf, nan, zero keep the
division's own answers"), restated in plain float64:
  * no reads: theta 1/K, log-likelihood 0, no iteration;
  * K == 1: theta 1, no iteration, log-likelihood of theta = 1;
  * a class with reads whose isoforms all have G = 0: s = 0, log 0 = -inf, the log-likelihood is -inf from the start,
    -inf / -inf is no number, no number is not > 1e-6: one iteration;
  * a log-likelihood of exactly 0: float64 reaches it where every mixture with reads ROUNDS to 1.0 (an isoform with
    ARS 1 taking every read), 40 digits would not for another hundred iterations.  The reference therefore takes the
    logarithm of a mixture as 0 where the mixture rounds to 1.0 in float64.  x / 0 is +-inf (> 1e-6: the loop goes on),
    0 / 0 is no number (the loop ends).  Where theta reaches (1, 0) in one step this is exact; where it only approaches it,
    the iteration at which float64 runs out of digits is decided by the rounding of theta itself, and two correct float64
    programs may differ by one (Trajectory.rounding_stop marks those events; the rule for them stays the exact one).
"""
import functools
import math
from decimal import Decimal, localcontext

import numpy as np

PREC = 40
THRESHOLD = 1e-6
W = 1e-9                   # 100 times the library's guard band of 1e-11 (lsq_set_em_guard_band)
REL_TOL = 1e-6             # the project's tolerance (tests/test_parity_gpu.py)
MAX_ITERS = 100000         # no case set comes near it

# The sharp bound.  Largest deviation of the plain float64 EM below (libm log, IEEE division) from the decimal reference
# over all case sets of this module, at equal iteration counts (tests/test_em_reference_host.py
# ::test_float64_em_stays_within_the_measured_deviation measures it again and holds it against these):
#   theta, absolute:            MEASURED_THETA_DEV -> SHARP_THETA_ABS = 2.4e-12
#   log-likelihood, relative:   MEASURED_LL_DEV    -> SHARP_LL_REL = min(4.3e-6, REL_TOL) = 1e-6
# The kernels get 1000 times that: their reciprocal and logarithm are good to about 1 ulp rather than half of one, and
# the log1p chain and the closed form add error over some hundreds of passes.  Never looser than REL_TOL.
# Measured: theta 2.36e-15 (lean set), log-likelihood 4.28e-9 -- the latter on the lean set's events with an ARS of 1 and
# 1e9 reads, (1e9, 1, 1e9) and (1, 1, 1e9): there a mixture of 1 - 1e-9 carries 1e9 reads, and its logarithm keeps seven
# digits of the sixteen; everywhere else it stays below 3e-12 (general sets: 6e-16).  Rounded up:
MEASURED_THETA_DEV = 2.4e-15
MEASURED_LL_DEV = 4.3e-9
SHARP_THETA_ABS = min(1000 * MEASURED_THETA_DEV, REL_TOL)
SHARP_LL_REL = min(1000 * MEASURED_LL_DEV, REL_TOL)

NAN = float("nan")
INF = float("inf")


def _pairs(K, ars, counts):
    """the (count, [isoforms of the class]) pairs with reads, per read file: [(m, k, [j...])]"""
    out = []
    for m, row in enumerate(counts):
        assert len(row) == (1 << K) - 1
        for c in range(1, 1 << K):
            k = int(row[c - 1])
            if k:
                out.append((m, k, [j for j in range(K) if c >> j & 1]))
    return out


class Trajectory:
    """theta[t], ll[t] (floats; -inf where it is) and crit[t] (float; nan / inf where IEEE gives those; crit[0] is None) for
    t = 0 .. len - 1, `stop`: the iteration at which the loop of read.h ends.  The trajectory runs on past `stop` while the
    test value is within W of the threshold, so that a flagged kernel result can be judged.  theta_dec / ll_dec: the
    40-digit values (ll_dec None where the log-likelihood is -inf)."""

    def __init__(self, K):
        self.K = K
        self.theta_dec, self.ll_dec, self.theta, self.ll, self.crit = [], [], [], [], []
        self.stop = 0
        self.rounding_stop = False         # the loop ended on a log-likelihood of exactly 0 (see the module's text)

    def near_threshold(self, upto=None):
        """some test value up to iteration `upto` (default: the last one kept) lies within W of the threshold"""
        last = len(self.crit) - 1 if upto is None else min(upto, len(self.crit) - 1)
        return any(self.crit[t] == self.crit[t] and abs(self.crit[t] - THRESHOLD) <= W for t in range(1, last + 1))


def _ll_dec(pairs, G, th):
    """the log-likelihood at th as a Decimal, None for -inf"""
    total = Decimal(0)
    for m, k, iso in pairs:
        s = sum((th[j] * G[m][j] for j in iso), Decimal(0))
        if s == 0:
            return None
        if float(s) == 1.0:
            continue                       # rounds to 1.0 in float64: log 1 = 0 (see the module's text)
        total += k * s.ln()
    return total


def _crit(old, new):
    """|1 - old / new| with the IEEE outcomes: None = -inf"""
    if new is None:
        return NAN if old is None else 1.0           # -inf / -inf: nan;  x / -inf = 0: |1 - 0|
    if old is None:
        return INF
    if new == 0:
        return NAN if old == 0 else INF
    return float(abs(1 - old / new))


def em_trajectory(K, ars, counts):
    """K isoforms, ars[m][j] (integers, 0 allowed), counts[m][class - 1] -> Trajectory"""
    with localcontext() as ctx:
        ctx.prec = PREC
        G = [[Decimal(0) if a == 0 else Decimal(1) / Decimal(int(a)) for a in row] for row in ars]
        pairs = _pairs(K, ars, counts)
        n = sum(k for _, k, _ in pairs)
        T = Trajectory(K)
        th = [Decimal(1) if K == 1 else Decimal(1) / Decimal(K)] * K

        def keep(th, ll, crit):
            T.theta_dec.append(list(th)); T.ll_dec.append(ll)
            T.theta.append([float(x) for x in th]); T.ll.append(-INF if ll is None else float(ll)); T.crit.append(crit)

        if n == 0:
            keep(th, Decimal(0), None)
            return T
        ll = _ll_dec(pairs, G, th)
        keep(th, ll, None)
        if K == 1:
            return T
        stopped = False
        for t in range(1, MAX_ITERS + 1):
            z = [Decimal(0)] * K
            for m, k, iso in pairs:
                s = sum((th[j] * G[m][j] for j in iso), Decimal(0))
                if s > 0:
                    for j in iso:
                        z[j] += k * (th[j] * G[m][j] / s)
            th = [x / n for x in z]
            nll = _ll_dec(pairs, G, th)
            c = _crit(ll, nll)
            ll = nll
            keep(th, ll, c)
            if not stopped and not (c > THRESHOLD):
                stopped = True
                T.stop = t
                T.rounding_stop = nll is not None and nll == 0
            if stopped and not (c > THRESHOLD - W):
                break                      # below the band: no admissible stop lies beyond
            if stopped and t >= T.stop + 64:
                break
        assert stopped, "the reference did not stop"
        return T


def em_float64(K, ars, counts, n_iters=None):
    """The plain float64 class-wise EM: libm's log (math.log), IEEE division, the sums in class order.  n_iters: run exactly
    that many iterations (for the deviation at equal iteration counts); None: until the stop test.  -> (theta, ll, iters)"""
    G = np.array([[0.0 if a == 0 else 1.0 / float(a) for a in row] for row in ars], np.float64)
    pairs = _pairs(K, ars, counts)
    n = float(sum(k for _, k, _ in pairs))
    th = np.full(K, 1.0 if K == 1 else 1.0 / K, np.float64)

    def loglik(th):
        total = 0.0
        for m, k, iso in pairs:
            s = 0.0
            for j in iso:
                s += float(th[j] * G[m][j])
            total += float(k) * (math.log(s) if s > 0 else -INF)
        return total

    if n == 0:
        return th, 0.0, 0
    ll = loglik(th)
    if K == 1:
        return th, ll, 0
    it = 0
    while True:
        z = np.zeros(K, np.float64)
        for m, k, iso in pairs:
            s = 0.0
            for j in iso:
                s += float(th[j] * G[m][j])
            if s > 0:
                for j in iso:
                    local = float(th[j] * G[m][j])
                    if local > 0:
                        z[j] += float(k) * (local / s)
        th = z / n
        nll = loglik(th)
        with np.errstate(all="ignore"):
            c = float(np.abs(np.float64(1.0) - np.float64(ll) / np.float64(nll)))
        ll = nll
        it += 1
        if n_iters is not None:
            if it >= n_iters:
                return th, ll, it
        elif not (c > THRESHOLD):
            return th, ll, it
        assert it < MAX_ITERS


def same_number(a, b):
    return a == b or (a != a and b != b)


def _within(a, b, bound):
    """|a - b| <= bound for finite numbers; -inf, inf and no number only match themselves"""
    return same_number(a, b) or (math.isfinite(a) and math.isfinite(b) and abs(a - b) <= bound)


def accept(T, theta, ll, iters, flags, sharp=True):
    """None when the kernel's (theta, ll, iters, flags) of one event is acceptable against trajectory T, else the reason."""
    iters, flags = int(iters), int(flags)
    if flags & 2:
        return "flag bit 1 (iteration cap) is set"
    if flags & 4:
        return "flag bit 2 (replayed) is set, and nothing is replayed"
    if flags & ~1:
        return "unknown flag bits %d" % flags
    if not flags & 1:
        if iters != T.stop:
            return "%d iterations, the reference stops at %d (test values there: %r)" % (iters, T.stop, T.crit[max(T.stop - 1, 0):T.stop + 2])
    else:
        if iters < 1 or iters >= len(T.crit):
            return "flagged, and %d iterations lie outside the trajectory (stop %d, kept %d)" % (iters, T.stop, len(T.crit) - 1)
        if not T.near_threshold(iters):
            return "flagged, but no test value up to iteration %d is within %g of the threshold" % (iters, W)
        for t in range(1, iters):
            if not (T.crit[t] > THRESHOLD - W):
                return "flagged; %d iterations, but the test value at %d is %r: the loop had to end there" % (iters, t, T.crit[t])
        if not (T.crit[iters] <= THRESHOLD + W):
            return "flagged; stopped at %d where the test value is %r" % (iters, T.crit[iters])
    want_theta, want_ll = T.theta[iters], T.ll[iters]
    for j, (a, b) in enumerate(zip(theta, want_theta)):
        a = float(a)
        if not _within(a, b, REL_TOL * max(abs(a), abs(b))):
            return "theta[%d] = %r, reference %r at iteration %d (REL_TOL)" % (j, a, b, iters)
        if sharp and not _within(a, b, SHARP_THETA_ABS):
            return "theta[%d] = %r, reference %r at iteration %d: off by %.3g, sharp bound %.3g" % (j, a, b, iters, abs(a - b), SHARP_THETA_ABS)
    ll = float(ll)
    if not _within(ll, want_ll, min(REL_TOL, SHARP_LL_REL if sharp else REL_TOL) * max(abs(ll), abs(want_ll))):
        return "log-likelihood %r, reference %r at iteration %d" % (ll, want_ll, iters)
    return None


# ---------------------------------------------------------------------------------------------------------- case sets

LEAN_READ_LENGTH = 100
# (name, exon length of isoform 0, of isoform 1): an isoform is one exon of its own, ARS = length - read length + 1
LEAN_STRUCTURES = [
    ("unequal", 300, 180),         # ARS 201, 81
    ("equal", 250, 250),           # ARS 151, 151: G0 == G1, the closed form's linear branch
    ("differ1", 250, 251),         # ARS 151, 152
    ("ratio100", 1099, 109),       # ARS 1000, 10
    ("ars1", 100, 150),            # ARS 1, 51: G0 = 1
    ("ars0", 60, 200),             # ARS 0, 101: G0 = 0
]
LEAN_ARS = {"unequal": (201, 81), "equal": (151, 151), "differ1": (151, 152), "ratio100": (1000, 10), "ars1": (1, 51), "ars0": (0, 101)}


def lean_triples():
    """(n1, n2, n3): reads on isoform 0 alone, on isoform 1 alone, on both"""
    t = [(0, 0, 0), (0, 0, 7), (0, 0, 1000), (5, 0, 0), (12345, 0, 0), (0, 3, 0), (0, 40000, 0),
         (3, 0, 5000), (40, 0, 10 ** 6), (0, 3, 5000), (0, 40, 10 ** 6),
         (1, 1, 10), (1, 1, 10 ** 3), (1, 1, 10 ** 6), (1, 1, 10 ** 9),
         (1, 1, 0), (250, 250, 0), (10 ** 5, 10 ** 5, 0), (1, 10 ** 9, 0), (10 ** 9, 1, 10 ** 9)]
    for big in (2 ** 31 - 1, 2 ** 31 + 1, 2 ** 32 - 1, 2 ** 32 + 1, 2 ** 40):
        t.append((big, 0, 0))
    t += [(0, 2 ** 31 + 1, 0), (0, 0, 2 ** 32 + 1), (0, 0, 2 ** 40), (0, 2 ** 40, 0)]
    # slow approaches: few reads on the isoforms alone under many on both (the iteration counts beyond 48 come from here)
    t += [(2, 1, 400), (3, 5, 2000), (7, 2, 30000), (30, 50, 10 ** 5), (1, 2, 50), (200, 100, 10 ** 6), (5, 9, 700), (11, 4, 9000)]
    rng = np.random.default_rng(20240611)
    while len(t) < 64:
        v = [0 if rng.random() < 0.3 else int(round(10 ** rng.uniform(0, 6))) for _ in range(3)]
        t.append(tuple(v))
    return t


def lean_cases():
    """[(gene name, structure name, (ars0, ars1), (n1, n2, n3))] in gene-name order: one event each"""
    out = []
    for s, (name, _, _) in enumerate(LEAN_STRUCTURES):
        for i, tr in enumerate(lean_triples()):
            out.append(("L%d_%s_%03d" % (s, name, i), name, LEAN_ARS[name], tr))
    return out


GENERAL_READ_LENGTHS = (100, 36, 75, 50, 90, 60, 40, 120)          # read file m of a context with M files: the first M
# exon lengths per isoform (one exon each, at least 121 long so that no ARS is 0 for any read length), K = 1 .. 6
GENERAL_STRUCTURES = [
    (300,), (260, 410), (500, 221, 350), (230, 777, 305, 412), (640, 233, 1250, 301, 455), (222, 518, 333, 999, 287, 404),
]
GENERAL_PATTERNS = ("zero", "all_iso", "singletons", "one_singleton", "ones", "sparse", "big", "file_empty")


def general_ars(lengths, M):
    return [[L - GENERAL_READ_LENGTHS[m] + 1 for L in lengths] for m in range(M)]


def general_counts(K, M, pattern, seed):
    nc = (1 << K) - 1
    cnt = [[0] * nc for _ in range(M)]
    rng = np.random.default_rng(seed)
    if pattern == "zero":
        pass
    elif pattern == "all_iso":
        for m in range(M):
            cnt[m][nc - 1] = 37 + 100 * m
    elif pattern == "singletons":
        for m in range(M):
            for j in range(K):
                cnt[m][(1 << j) - 1] = 3 + 5 * j + 11 * m
    elif pattern == "one_singleton":
        cnt[M - 1][(1 << (K - 1)) - 1] = 19
    elif pattern == "ones":
        for m in range(M):
            cnt[m] = [1] * nc
    elif pattern == "sparse":
        for m in range(M):
            for c in range(nc):
                if rng.random() < 0.3:
                    cnt[m][c] = int(round(10 ** rng.uniform(0, 6)))
        cnt[0][nc - 1] += 1
    elif pattern == "big":
        cnt[0][nc - 1] = 2 ** 32 + 1
        for m in range(M):
            for j in range(K):
                cnt[m][(1 << j) - 1] += 1000 * (j + 1)
    elif pattern == "file_empty":
        for m in range(1, M):
            for c in range(nc):
                if rng.random() < 0.5:
                    cnt[m][c] = int(rng.integers(1, 500))
        if M == 1:
            pass                           # the one read file is the empty one: no reads at all
    else:
        raise ValueError(pattern)
    return cnt


def general_cases(M):
    """[(gene name, K, exon lengths, ars[m][j], counts[m][c])] in gene-name order"""
    out = []
    for K, lengths in enumerate(GENERAL_STRUCTURES, 1):
        for p, pattern in enumerate(GENERAL_PATTERNS):
            out.append(("G%d_%s" % (K, pattern), K, lengths, general_ars(lengths, M), general_counts(K, M, pattern, 1000 * M + 10 * K + p)))
    out.sort(key=lambda r: r[0])
    return out


def write_annotation(directory, stem, genes):
    """genes: [(gene name, [exon length per isoform])] -> (<stem>.interval, <stem>.map) paths: every isoform is one exon of
    its own on chr1 +, no two overlap (a single-exon isoform of length L has ARS L - read length + 1, 0 when that is negative).
    An isoform given as a list of (start, end) pairs instead of a length has those exons, counted from the first base of the
    gene's own stretch of 16 000 bases (tests/fim_ref.py: isoforms that share segments)."""
    import os
    from golden_inputs import interval_line
    iv, mp = [], []
    for g, (name, lengths) in enumerate(genes):
        for j, length in enumerate(lengths):
            if isinstance(length, (list, tuple)):
                base = 1000 + g * 16000
                assert all(0 <= s < e <= 15000 for s, e in length), (name, length)
                exons = [(base + s, base + e) for s, e in length]
            else:
                start = 1000 + (g * 8 + j) * 2000
                exons = [(start, start + length)]
            iv.append(interval_line("%s.i%d" % (name, j), "chr1", "+", exons))
            mp.append("%s\t%s.i%d\n" % (name, name, j))
    a, b = os.path.join(directory, stem + ".interval"), os.path.join(directory, stem + ".map")
    with open(a, "w") as f:
        f.write("".join(iv))
    with open(b, "w") as f:
        f.write("".join(mp))
    return a, b


def lean_genes():
    lengths = {name: (a, b) for name, a, b in LEAN_STRUCTURES}
    return [(gname, list(lengths[sname])) for gname, sname, _, _ in lean_cases()]


def general_genes(M):
    return [(gname, list(lengths)) for gname, _, lengths, _, _ in general_cases(M)]


def trajectories(cases_kac):
    """[(K, ars, counts)] -> [Trajectory]"""
    return [em_trajectory(K, ars, counts) for K, ars, counts in cases_kac]


def lean_kac():
    return [(2, [list(ars)], [list(tr)]) for _, _, ars, tr in lean_cases()]


def general_kac(M):
    return [(K, ars, counts) for _, K, _, ars, counts in general_cases(M)]


# computed once per process, shared by every test that needs them, never changed
@functools.lru_cache(maxsize=None)
def lean_trajectories():
    return tuple(trajectories(lean_kac()))


@functools.lru_cache(maxsize=None)
def general_trajectories(M):
    return tuple(trajectories(general_kac(M)))
