"""The reference of the read bootstrap's resampling, written from the definition and not from the C++: a
vectorised numpy Philox4x32-10 and the draw -> class rule.  No GPU, no library call.

A replicate resamples the counted reads of each (read file m, event e) with replacement and keeps that pair's total n:
draw i = 0 .. n - 1 of replicate b takes the Philox block of counter (j low word, j high word, e, (m << 24) | b), j = i >> 1,
under key (seed low word, seed high word); even i uses u = x0 | x1 << 32, odd i uses u = x2 | x3 << 32; r = (u * n) >> 64;
the class drawn is the smallest c whose inclusive cumulative count exceeds r."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four arrays (or integers) of 32-bit words, key: two -> four uint64 arrays holding the 32-bit output words"""
    c = [np.atleast_1d(np.asarray(x, np.uint64)) & MASK32 for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for rnd in range(10):
        if rnd:
            k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
        p0 = np.uint64(M0) * c[0]              # 32 x 32 bits: fits 64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
    return c


def mul_hi(u, n):
    """(u * n) >> 64 for a uint64 array u and an integer n < 2^64, by 32-bit limbs"""
    n = int(n)
    u = np.asarray(u, np.uint64)
    s32 = np.uint64(32)
    ul, uh = u & MASK32, u >> s32
    nl, nh = np.uint64(n & 0xFFFFFFFF), np.uint64(n >> 32)
    ll, lh, hl, hh = ul * nl, ul * nh, uh * nl, uh * nh
    mid = (ll >> s32) + (lh & MASK32) + (hl & MASK32)
    return hh + (lh >> s32) + (hl >> s32) + (mid >> s32)


def draws(counts, seed, m, e, b, first=0, n_draws=None):
    """the classes (1-based) of the draws first .. first + n_draws - 1 (default: all of them) of one (read file m, event e)"""
    counts = [int(x) for x in counts]
    n = sum(counts)
    if n_draws is None:
        n_draws = n - first
    assert 0 <= first and first + n_draws <= n and b < 2 ** 24
    if n_draws == 0:
        return np.zeros(0, np.uint32)
    # one block per pair of draws: the blocks j0 .. j1, their two halves interleaved, cut to the draws asked for
    j0, j1 = first >> 1, (first + n_draws - 1) >> 1
    j = np.arange(j0, j1 + 1, dtype=np.uint64)
    x = philox4x32_10((j & MASK32, j >> np.uint64(32), e, (m << 24) | b), (seed & 0xFFFFFFFF, seed >> 32))
    u = np.empty(2 * len(j), np.uint64)
    u[0::2] = x[0] | (x[1] << np.uint64(32))            # even i
    u[1::2] = x[2] | (x[3] << np.uint64(32))            # odd i
    u = u[first - 2 * j0:first - 2 * j0 + n_draws]
    r = mul_hi(u, n)
    cum = np.cumsum(np.array(counts, dtype=object)).astype(np.uint64)      # (n < 2^64)
    # the smallest c with cum[c] > r: the number of entries <= r
    return (np.searchsorted(cum, r, side="right") + 1).astype(np.uint32)


def resample(class_off, class_count, seed, b):
    """replicate b's counts of every (read file, event): class_count[m, slot] in the layout of class_off -> the same shape"""
    class_count = np.asarray(class_count, np.uint64)
    out = np.zeros_like(class_count)
    for m in range(class_count.shape[0]):
        for e in range(len(class_off) - 1):
            a, z = int(class_off[e]), int(class_off[e + 1])
            cls = draws(class_count[m, a:z], seed, m, e, b)
            if len(cls):
                out[m, a:z] = np.bincount(cls - 1, minlength=z - a).astype(np.uint64)
    return out
