"""The reference of the direct Fisher information tests: the expected Fisher information of common/fim.h and the two
variance estimates made from it, from the definition, in exact rational arithmetic (fractions.Fraction); the bounds a
float64 evaluation has to keep against it; and the case set of tests/test_fim_reference_host.py and
tests/test_fim_direct_gpu.py.  No GPU, no library call: pure Python.

The definition (fim.h:115-158 bruteforce_fim, :320-367 ofim; restated in double precision by oracle/lsq_oracle.c).  An
event has segments of given lengths and K isoforms, each a set of segments; a read file has a read length R and a read
type.  For every isoform k with theta_k != 0, every accessible read start of k is visited, ONE AT A TIME:
  * accessible starts (oracle/lsq_oracle.c fim_ars_lengths): walking k's segments with c the length walked so far
    (this segment included) and L the isoform's length, a segment of length l contributes the starts [c - l, c - l + a)
    in isoform coordinates, a = l (MEDIUM_READ) or l + 1 (SHORT_READ: the last of them is the first base of the next
    segment, which that segment contributes again -- it is visited twice), up to the first segment with c + R > L, where
    less than a read is left: that one contributes a = max(l + 1 - (c + R - L), 0), and no segment after it anything;
  * the read generated at start x covers k's segments from the one that holds base x to the one that holds base
    x + R - 1;
  * it is compatible with isoform j when its segments are a run of consecutive entries of j's segment list (the
    connected-compatibility rule); dG_j = G_j if compatible, else 0;
  * s = sum of theta_j dG_j over the j with dG_j > 0 and theta_j > 0;
  * the start's term for entry (p, q), p, q < D = K - 1, is theta_k G_k (dG_p - dG_K)(dG_q - dG_K) / s^2, K the last isoform.
I_pq is the sum of the terms, A_pq the sum of their absolute values.  theta and G enter as the exact values of the doubles
given (Fraction(float) is exact).  Nothing is counted in runs or by classes: a start adds its numerator to the bucket of
its own denominator s^2 -- the same sum, only brought over few common denominators instead of one of some thousand bits
per addition --, and the number of starts per (isoform, class) is kept beside it for the counting tests.

by_diag = sum_p 1 / I_pp (fim.h:64-72; inf where a diagonal entry is 0), by_inv = the sum of all entries of the inverse
plus its trace (fim.h:74-93); det and the inverse are exact (rational Gauss-Jordan).

THE BOUNDS.  eps = 2^-53, T = the number of (isoform, class) groups with starts among the isoforms with theta != 0,
C1 = 4 (T + 2 K + 10).

matrix: |got - I_pq| <= C1 eps A_pq.  A float64 evaluation forms a group's term as n theta_k G_k dp dq / s^2.  s is a sum of
at most K products of positive numbers: each product carries its own rounding and at most K - 1 of the additions', so s is
good to K eps relative and s^2 to 2 K eps plus the square's own rounding.  Further: theta_k G_k 1, times n 1, the quotient 1,
dp and dq (differences of two exact doubles) 1 each, the two products with them 2: 2 K + 8 roundings a term,
(2 K + 8) eps |term| to first order.  Adding T such terms into one accumulator costs at most (T - 1) eps of the sum of their
absolute values.  Together (T + 2 K + 7) eps A_pq <= (T + 2 K + 10) eps A_pq; the factor 4 is slack for second-order terms, fused
multiply-adds and another order of the operations.

by_diag: relative (C1 + D + 2) eps.  Every term of a diagonal entry is >= 0, so A_pp = I_pp and the entry is good to
C1 eps relative; its reciprocal adds 1, the sum of D non-negative numbers at most D - 1, one to spare.

by_inv: |got - by_inv| <= (C1 + 3 D^3 2^(D-1)) eps kappa S, kappa = ||I||_inf ||I^-1||_inf, S = sum_ij |I^-1_ij| + sum_i |I^-1_ii|.
First part, the matrix that goes in: it is I + E with |E_pq| <= C1 eps A_pq, the inverse changes by - I^-1 E I^-1 to first
order, and a relative change of C1 eps in the matrix is a relative change of at most kappa C1 eps in the inverse, which
enters by_inv through S.  (This takes ||E|| <= C1 eps ||I||, that is A_pq for |I_pq|: exact on the diagonal, where no term
cancels; off it |A_pq| <= sqrt(I_pp I_qq) by Cauchy-Schwarz, so ||A||_inf <= D ||I||_inf at the worst, and the slack of 4
in C1 is what stands against that.)  Second part, the inversion itself: Gaussian elimination with partial pivoting
solves each column of the identity with a forward error of at most 3 D^3 rho eps kappa relative in norm (Higham, Accuracy
and Stability of Numerical Algorithms, theorem 9.5 with gamma_D ~ D eps and ||L|| ||U|| <= D^2 rho ||I||), growth factor
rho <= 2^(D-1); again through S.
"""
import functools
import math
import random
from fractions import Fraction

EPS = Fraction(1, 2 ** 53)
INF = float("inf")


# ------------------------------------------------------------------------------------------------------ the definition

def accessible_start_lengths(seg_len, R, short):
    """seg_len: the lengths of ONE isoform's segments in order -> the number of accessible starts each contributes"""
    L = sum(seg_len)
    out, c = [], 0
    for i, l in enumerate(seg_len):
        c += l
        if c + R > L:                                   # less than a read is left behind this segment's end
            out.append(max(l + 1 - (c + R - L), 0))
            return out + [0] * (len(seg_len) - i - 1)
        out.append(l + 1 if short else l)
    return out


def accessible_starts(seg_len, R, short):
    """the accessible starts of one isoform in isoform coordinates, one entry a start (SHORT_READ: a boundary start twice)"""
    out, before = [], 0
    for l, a in zip(seg_len, accessible_start_lengths(seg_len, R, short)):
        out.extend(before + t for t in range(a))
        before += l
    return out


def generated_read(seg_len, start, R):
    """(first, last): the places in the isoform's segment list of the segments that hold base `start` and base start + R - 1"""
    first = last = None
    lo = 0
    for i, l in enumerate(seg_len):
        if lo <= start < lo + l:
            first = i
        if lo <= start + R - 1 < lo + l:
            last = i
        lo += l
    assert first is not None and last is not None, "a start from which no whole read fits (the reference asserts)"
    return first, last


def compatible(read, iso):
    """connected compatibility: the read's segments are a run of consecutive entries of the isoform's segment list"""
    n = len(read)
    return any(iso[j:j + n] == read for j in range(len(iso) - n + 1))


def _scaled(values):
    """Fractions -> (integers, den) with value = integer / den"""
    den = 1
    for v in values:
        den = den * v.denominator // math.gcd(den, v.denominator)
    return [int(v * den) for v in values], den


class Fim:
    """K, D, I and A (D x D lists of Fractions), T, starts[k] ({class: number of starts}), by_diag (Fraction, or inf), det,
    and where det != 0: inv, by_inv, norm, norm_inv, kappa, S"""

    def c1(self):
        return 4 * (self.T + 2 * self.K + 10)

    def matrix_bound(self, p, q):
        return self.c1() * EPS * self.A[p][q]

    def by_diag_rel_bound(self):
        return (self.c1() + self.D + 2) * EPS

    def by_inv_bound(self):
        D = self.D
        return (self.c1() + 3 * D ** 3 * 2 ** (D - 1)) * EPS * self.kappa * self.S if D else Fraction(0)

    def by_inv_rel_bound(self):
        """the by_inv bound relative to |by_inv| as a float (inf where by_inv is 0)"""
        if self.D == 0:
            return 0.0
        return float(self.by_inv_bound() / abs(self.by_inv)) if self.by_inv != 0 else INF


def fim(seg_len, isoforms, R, short, theta, G):
    """seg_len[n]: the event's segment lengths; isoforms[j]: ascending list of segment indices; theta[j], G[j]: floats (taken
    exactly) or Fractions -> Fim"""
    K, D = len(isoforms), len(isoforms) - 1
    isoforms = [list(x) for x in isoforms]
    th = [Fraction(x) for x in theta]
    g = [Fraction(x) for x in G]
    assert len(th) == len(g) == K and all(x >= 0 for x in th) and all(x >= 0 for x in g)
    tn, tden = _scaled(th)
    gn, gden = _scaled(g)
    num, absnum = {}, {}                       # sn -> D x D integer numerators (upper triangle), plain and absolute
    starts = [dict() for _ in range(K)]
    groups = set()
    for k in range(K):
        lens = [seg_len[n] for n in isoforms[k]]
        for x in accessible_starts(lens, R, short):
            first, last = generated_read(lens, x, R)
            read = isoforms[k][first:last + 1]
            comp = [compatible(read, isoforms[j]) for j in range(K)]
            cls = sum(1 << j for j in range(K) if comp[j])
            starts[k][cls] = starts[k].get(cls, 0) + 1
            if th[k] == 0:
                continue
            groups.add((k, cls))
            dg = [gn[j] if comp[j] else 0 for j in range(K)]
            sn = sum(tn[j] * dg[j] for j in range(K) if dg[j] > 0 and tn[j] > 0)
            assert sn > 0
            w = tn[k] * gn[k]
            if sn not in num:
                num[sn] = [[0] * D for _ in range(D)]
                absnum[sn] = [[0] * D for _ in range(D)]
            a, b = num[sn], absnum[sn]
            d = [dg[p] - dg[K - 1] for p in range(D)]
            for p in range(D):
                if d[p]:
                    wp = w * d[p]
                    for q in range(p, D):
                        t = wp * d[q]
                        a[p][q] += t
                        b[p][q] += abs(t)
    # term = theta_k G_k dp dq / s^2 = (tn_k gn_k dpn dqn / sn^2) * tden / gden
    scale = Fraction(tden, gden)
    F = Fim()
    F.K, F.D, F.T, F.starts = K, D, len(groups), starts
    F.I = [[Fraction(0)] * D for _ in range(D)]
    F.A = [[Fraction(0)] * D for _ in range(D)]
    for sn in num:
        for p in range(D):
            for q in range(p, D):
                if absnum[sn][p][q]:
                    F.I[p][q] += Fraction(num[sn][p][q], sn * sn)
                    F.A[p][q] += Fraction(absnum[sn][p][q], sn * sn)
    for p in range(D):
        for q in range(p, D):
            F.I[p][q] *= scale
            F.A[p][q] *= scale
            F.I[q][p], F.A[q][p] = F.I[p][q], F.A[p][q]
    F.by_diag = INF if any(F.I[p][p] == 0 for p in range(D)) else sum((1 / F.I[p][p] for p in range(D)), Fraction(0))
    F.det, F.inv = _det_and_inverse(F.I)
    if F.det != 0:
        F.by_inv = sum((x for row in F.inv for x in row), Fraction(0)) + sum((F.inv[i][i] for i in range(D)), Fraction(0))
        F.norm = max((sum(abs(x) for x in row) for row in F.I), default=Fraction(0))
        F.norm_inv = max((sum(abs(x) for x in row) for row in F.inv), default=Fraction(0))
        F.kappa = F.norm * F.norm_inv
        F.S = sum((abs(x) for row in F.inv for x in row), Fraction(0)) + sum((abs(F.inv[i][i]) for i in range(D)), Fraction(0))
    return F


def _det_and_inverse(M):
    """exact determinant and, where it is not 0, the inverse: Gauss-Jordan on Fractions (the empty matrix: 1 and [])"""
    D = len(M)
    a = [list(M[i]) + [Fraction(int(i == j)) for j in range(D)] for i in range(D)]
    det = Fraction(1)
    for c in range(D):
        piv = next((r for r in range(c, D) if a[r][c] != 0), None)
        if piv is None:
            return Fraction(0), None
        if piv != c:
            a[c], a[piv] = a[piv], a[c]
            det = -det
        det *= a[c][c]
        inv_p = 1 / a[c][c]
        a[c] = [x * inv_p for x in a[c]]
        for r in range(D):
            if r != c and a[r][c] != 0:
                f = a[r][c]
                a[r] = [x - f * y for x, y in zip(a[r], a[c])]
    return det, [row[D:] for row in a]


def row_exchanges(M):
    """the number of row exchanges of Gaussian elimination with partial pivoting on M, in exact arithmetic"""
    D = len(M)
    a = [list(r) for r in M]
    n = 0
    for j in range(D - 1):
        ip = j
        for i in range(j + 1, D):
            if abs(a[i][j]) > abs(a[ip][j]):
                ip = i
        if ip != j:
            a[j], a[ip] = a[ip], a[j]
            n += 1
        if a[j][j] != 0:
            for i in range(j + 1, D):
                f = a[i][j] / a[j][j]
                a[i] = [x - f * y for x, y in zip(a[i], a[j])]
    return n


def error_ratio(got, exact, bound):
    """|got - exact| / bound as a float for a float64 `got`: 0 where both agree exactly, inf where a bound of 0 is missed or
    `got` is no finite number"""
    if not math.isfinite(got):
        return INF
    err = abs(Fraction(got) - exact)
    if err == 0:
        return 0.0
    return float(err / bound) if bound > 0 else INF


# ------------------------------------------------------------------------------------------------------------ geometry

def segmentation(isoform_exons):
    """isoform_exons[j]: [(start, end)] -> (segments [(start, end)], isoforms [[segment index]]): the atomic intervals between
    neighbouring exon boundaries that some exon covers"""
    cuts = sorted({x for ex in isoform_exons for se in ex for x in se})
    segs = [(a, b) for a, b in zip(cuts, cuts[1:]) if any(s <= a and b <= e for ex in isoform_exons for s, e in ex)]
    isoforms = [[n for n, (a, b) in enumerate(segs) if any(s <= a and b <= e for s, e in ex)] for ex in isoform_exons]
    return segs, isoforms


EDGES = ("segment_shorter_than_R", "segment_of_length_1", "isoform_of_length_R", "isoform_shorter_than_R",
         "ends_in_the_segment_where_less_than_a_read_is_left", "segments_behind_the_one_where_less_than_a_read_is_left")


def geometry_edges(seg_len, isoforms, R):
    """which of EDGES the event has for read length R"""
    out = set()
    for iso in isoforms:
        lens = [seg_len[n] for n in iso]
        L = sum(lens)
        if any(l < R for l in lens):
            out.add(EDGES[0])
        if 1 in lens:
            out.add(EDGES[1])
        if L == R:
            out.add(EDGES[2])
        if L < R:
            out.add(EDGES[3])
            continue
        c = 0
        for i, l in enumerate(lens):
            c += l
            if c + R > L:
                out.add(EDGES[4] if i == len(lens) - 1 else EDGES[5])
                break
    return out


# ------------------------------------------------------------------------------------------------------ the direct set

READ_FILES = (("SHORT_READ", 10), ("MEDIUM_READ", 36))          # (read type, read length) of the set's two read files
PATTERNS = ("balanced", "big", "zero_mid", "zero_last", "shared")

# the hand-made structures: (name, exons per isoform[, count patterns]), coordinates from the gene's first base
HAND = [
    ("one_exon", [[(0, 80)]]),
    ("one_two_exons", [[(0, 30), (100, 150)]]),
    ("one_short", [[(0, 12), (40, 52)]]),                                    # 24 bases: no start for reads of 36
    ("cassette", [[(0, 40), (100, 125), (200, 250)], [(0, 40), (200, 250)]]),
    ("cassette_of_1", [[(0, 44), (100, 101), (200, 251)], [(0, 44), (200, 251)]]),                # a segment of length 1
    ("cassette_of_7", [[(0, 38), (100, 107), (200, 247)], [(0, 38), (200, 247)]]),                # shorter than either read
    ("alt5", [[(0, 50), (200, 260)], [(0, 65), (200, 260)]]),
    ("alt3", [[(0, 55), (200, 262)], [(0, 55), (180, 262)]]),
    ("mxe", [[(0, 45), (100, 130), (300, 350)], [(0, 45), (200, 222), (300, 350)]]),
    ("retained_intron", [[(0, 140)], [(0, 50), (90, 140)]]),
    ("exactly_a_read", [[(0, 4), (100, 106)], [(0, 4), (50, 90), (100, 106)]]),                   # 10 bases: one start for reads of 10
    ("exactly_36", [[(0, 20), (100, 116)], [(0, 20), (60, 75), (100, 116), (150, 170)]]),         # 36 bases: one start for reads of 36
    ("shorter_than_both", [[(0, 5), (100, 103)], [(0, 5), (50, 95), (100, 103), (150, 200)]], "BMS"),    # 8 bases: G = 0 in both files
    ("tail_behind", [[(0, 60), (100, 103), (200, 204)], [(0, 60), (200, 204), (300, 340)]]),      # short segments behind the last start
    ("two_cassettes", [[(0, 40), (100, 130), (200, 221), (300, 345)], [(0, 40), (100, 130), (300, 345)], [(0, 40), (300, 345)]]),
    ("alt5_three_sites", [[(0, 40), (200, 250)], [(0, 52), (200, 250)], [(0, 71), (200, 250)]]),
    ("mxe_or_skip", [[(0, 42), (100, 133), (300, 351)], [(0, 42), (200, 219), (300, 351)], [(0, 42), (300, 351)]]),
    ("retained_or_cassette", [[(0, 150)], [(0, 50), (100, 150)], [(0, 50), (70, 83), (100, 150)]]),
    ("alt3_three_sites", [[(0, 48), (200, 255)], [(0, 48), (187, 255)], [(0, 48), (164, 255)]]),
    ("cassette_in_a_retained_intron", [[(0, 160)], [(0, 45), (110, 160)], [(0, 45), (70, 79), (110, 160)]], "BGM"),     # (see RANDOM)
    # (the exon between the two cassettes is shorter than either read: a read joins them, the four isoforms can be told apart)
    ("independent_cassettes", [[(0, 40), (100, 125), (200, 206), (300, 318), (400, 450)], [(0, 40), (200, 206), (300, 318), (400, 450)],
                               [(0, 40), (100, 125), (200, 206), (400, 450)], [(0, 40), (200, 206), (400, 450)]]),
    ("alt_ends", [[(0, 60), (200, 247)], [(0, 60), (300, 361)], [(100, 133), (200, 247)], [(100, 133), (300, 361)]]),
]
# one class carries every start of the one isoform with theta != 0: the matrix is a rank-one outer product (D = 2 and 4)
SINGULAR = [
    ("singular_d2", [[(0, 50)], [(0, 50), (100, 130)], [(0, 50), (200, 275)]]),
    ("singular_d4", [[(0, 50)], [(0, 50), (100, 130)], [(0, 50), (200, 275)], [(0, 50), (100, 130), (300, 341)], [(0, 50), (200, 275), (400, 418)]]),
]


# the seeded random structures: (K, seed, count patterns).  Seeds and patterns are chosen so that no matrix of the set comes
# near 1 / eps in condition unless it is singular exactly (tests/test_fim_reference_host.py asserts that): reads on the shared
# class alone drive theta to a vertex, and with most structures the matrix there is singular to float64.
RANDOM = [
    (4, 0, "BGS"), (4, 1, "BGL"), (4, 3, "GMS"), (4, 4, "BMS"), (4, 6, "GLS"), (4, 7, "BML"), (4, 17, "BGS"), (4, 22, "MLS"), (4, 23, "BGS"),
    (5, 0, "BLG"), (5, 1, "BGS"), (5, 2, "MLS"), (5, 3, "BGS"), (5, 7, "GML"), (5, 12, "BMS"), (5, 21, "GLS"), (5, 22, "BMS"), (5, 23, "GLS"),
    (5, 14, "BGM"),
    (6, 2, "BGS"), (6, 3, "MLS"), (6, 5, "BGS"), (6, 8, "BGM"), (6, 9, "MLS"), (6, 13, "BGS"), (6, 16, "GLS"), (6, 20, "BMS"), (6, 21, "GMS"),
    (6, 22, "BLS"),
]
LETTER = {"B": "balanced", "G": "big", "M": "zero_mid", "L": "zero_last", "S": "shared"}


def random_structure(K, seed):
    """K distinct isoforms, random subsets of at most 8 segments of lengths 1 .. 60, seven bases between two segments"""
    rng = random.Random(1000 * K + seed)
    n = rng.randint(4, 8)
    lens = [rng.randint(1, 60) for _ in range(n)]
    pos, where = 0, []
    for l in lens:
        where.append((pos, pos + l))
        pos += l + 7
    subsets = set()
    while len(subsets) < K:
        s = tuple(i for i in range(n) if rng.random() < 0.6)
        if s:
            subsets.add(s)
    return [[where[i] for i in s] for s in sorted(subsets, key=lambda s: rng.random())]


class Case:
    """name, structure, K, exons[j], pattern, segments, seg_len, isoforms (from segmentation), ars[m][j], counts[m][class - 1]"""


def counts_of(K, ars, pattern, i):
    """the class counts of one event per read file.  Reads go to the classes of one isoform alone and to classes of many; a
    file in which an isoform has no accessible start (G = 0) carries no read on that isoform alone."""
    nc = (1 << K) - 1
    M = len(ars)
    cnt = [[0] * nc for _ in range(M)]
    alive = [[j for j in range(K) if ars[m][j] > 0] for m in range(M)]
    if K == 1:
        for m in range(M):
            if alive[m]:
                cnt[m][0] = 5 + i % 7 + 3 * m
        return cnt
    if pattern == "singular":
        for m in range(M):
            cnt[m][0] = 50 + 20 * m
    elif pattern == "balanced":
        for m in range(M):
            for j in alive[m]:
                cnt[m][(1 << j) - 1] = 40 + 3 * j + 11 * m + i % 5
            if alive[m]:
                cnt[m][nc - 1] = 25 + i % 3
    elif pattern == "big":
        for m in range(M):
            for j in alive[m]:
                cnt[m][(1 << j) - 1] = 1
        j0 = i % K if i % K in alive[0] else alive[0][0]
        cnt[0][(1 << j0) - 1] = 2 ** 40
    elif pattern in ("zero_mid", "zero_last"):
        k0 = (K - 1) // 2 if pattern == "zero_mid" else K - 1
        for m in range(M):
            for j in alive[m]:
                if j != k0:
                    cnt[m][(1 << j) - 1] = 30 + 5 * j + 2 * m + i % 4
            if K >= 3 and any(j != k0 for j in alive[m]):
                cnt[m][(nc ^ (1 << k0)) - 1] = 20            # the class of all the others
    elif pattern == "shared":
        for m in range(M):
            if alive[m]:
                cnt[m][nc - 1] = 500 + 100 * m + i
    else:
        raise ValueError(pattern)
    return cnt


@functools.lru_cache(maxsize=None)
def direct_set():
    """the direct set in gene-name (= output) order: events of different K interleaved, every structure under three count
    patterns (the hand-made ones: the patterns rotate; the random ones: RANDOM), the two singular structures under their own"""
    by_K = {}
    for n, (name, exons, *letters) in enumerate(HAND):
        K = len(exons)
        for r in range(1 if K == 1 else 3):
            by_K.setdefault(K, []).append((name, exons, LETTER[letters[0][r]] if letters else PATTERNS[(n + r) % len(PATTERNS)]))
    for K, seed, letters in RANDOM:
        for x in letters:
            by_K.setdefault(K, []).append(("random_k%d_%d" % (K, seed), random_structure(K, seed), LETTER[x]))
    for name, exons in SINGULAR:
        by_K[len(exons)].append((name, exons, "singular"))
    dealt = []                                  # one of each K in turn, as long as there are any
    while any(by_K.values()):
        for K in sorted(by_K):
            if by_K[K]:
                dealt.append(by_K[K].pop(0))
    out = []
    for i, (name, exons, pattern) in enumerate(dealt):
        c = Case()
        c.K, c.structure, c.exons, c.pattern = len(exons), name, exons, pattern
        c.name = "F%03d_k%d_%s_%s" % (i, c.K, name, pattern)
        c.segments, c.isoforms = segmentation(exons)
        c.seg_len = [e - s for s, e in c.segments]
        c.ars = [[len(accessible_starts([c.seg_len[n] for n in iso], R, rt == "SHORT_READ")) for iso in c.isoforms] for rt, R in READ_FILES]
        c.counts = counts_of(c.K, c.ars, pattern, i)
        out.append(c)
    return tuple(out)


def direct_genes():
    """the set for em_ref.write_annotation: the genes lie on the chromosome in another order than their names'"""
    cases = list(direct_set())
    random.Random(5).shuffle(cases)
    return [(c.name, c.exons) for c in cases]


def G_of(ars):
    """1.0 / ARS in float64, 0 for ARS 0: what the library makes of the accessible read starts"""
    return [0.0 if a == 0 else 1.0 / float(a) for a in ars]


def reference_at(case, m, theta):
    """the exact reference of one event and read file of the set at the given theta (floats)"""
    rt, R = READ_FILES[m]
    return fim(case.seg_len, case.isoforms, R, rt == "SHORT_READ", theta, G_of(case.ars[m]))


def coverage(cases, thetas, refs):
    """cases of the set, thetas[e] (floats), refs[e][m] (Fim at that theta): asserts what keeps a test on the set from hiding a
    failure, by counting; returns the counts"""
    M = len(READ_FILES)
    assert len(cases) == len(thetas) == len(refs) and all(len(r) == M for r in refs)
    assert (len(cases) * M) % 64 != 0 and len(cases) * M > 4 * 64          # lanes of several workgroups, the last one ragged
    assert len({c.name for c in cases}) == len(cases) and [c.name for c in cases] == sorted(c.name for c in cases)
    assert all(a.K != b.K for a, b in zip(cases, cases[1:])), "neighbours in output order differ in K"
    per_K = {(K, m): sum(1 for c in cases if c.K == K) for K in range(1, 7) for m in range(M)}
    assert all(n >= 3 for n in per_K.values()), per_K
    edges = {e: 0 for e in EDGES}
    for c in cases:
        for m, (_, R) in enumerate(READ_FILES):
            for e in geometry_edges(c.seg_len, c.isoforms, R):
                edges[e] += 1
    assert all(n >= 1 for n in edges.values()), edges
    assert any(0 in ars for c in cases for ars in c.ars) and any(1 in ars for c in cases for ars in c.ars)          # G = 0, G = 1
    n_zero_mid = n_zero_last = n_big = n_shared = 0
    for c, th in zip(cases, thetas):
        assert len(th) == c.K and all(math.isfinite(x) and x >= 0 for x in th), (c.name, th)
        if c.K == 1:
            continue
        if c.pattern == "zero_mid":
            assert th[(c.K - 1) // 2] == 0, (c.name, th)
            n_zero_mid += 1
        elif c.pattern == "zero_last":
            assert th[c.K - 1] == 0, (c.name, th)
            n_zero_last += 1
        elif c.pattern == "big":
            assert 0 < min(x for x in th if x > 0) < 1e-11, (c.name, th)
            n_big += 1
        elif c.pattern == "shared":
            assert all(x == 0 for x in c.counts[0][:-1]) and c.counts[0][-1] > 0
            n_shared += 1
    assert min(n_zero_mid, n_zero_last, n_big, n_shared) >= 10
    singular = [(c.name, m) for c, r in zip(cases, refs) for m in range(M) if c.K > 1 and r[m].det == 0]
    regular = [(c, m, r[m]) for c, r in zip(cases, refs) for m in range(M) if c.K > 1 and r[m].det != 0]
    for name, D in (("singular_d2", 2), ("singular_d4", 4)):
        hit = [c for c in cases if c.structure == name]
        assert len(hit) == 1 and hit[0].K == D + 1 and all((hit[0].name, m) in singular for m in range(M)), name
    assert any(r[m].by_diag == INF for c, r in zip(cases, refs) for m in range(M) if c.K > 1)
    # an exactly regular matrix stays regular to float64: no condition number near 1 / eps (the bound is a first-order one)
    worst = max(f.kappa for _, _, f in regular)
    assert worst < 2 ** 50, float(worst)
    strict = sum(1 for _, _, f in regular if f.by_inv_rel_bound() < 1e-9)
    assert 3 * strict >= 2 * len(regular), (strict, len(regular))
    assert {f.D for _, _, f in regular if f.by_inv_rel_bound() < 1e-9} == {1, 2, 3, 4, 5}
    # the LU has rows to exchange at D = 4 and D = 5: a pivoting slip there changes a strict case's by_inv
    exchanged = {D: sum(1 for _, _, f in regular if f.D == D and f.by_inv_rel_bound() < 1e-9 and row_exchanges(f.I) > 0) for D in (4, 5)}
    assert all(n >= 3 for n in exchanged.values()), exchanged
    return dict(events=len(cases), regular=len(regular), strict=strict, singular=len(singular), worst_kappa=float(worst), edges=edges,
                row_exchanges=exchanged)
