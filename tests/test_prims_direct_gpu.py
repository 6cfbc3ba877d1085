"""The device prefix sum (csrc/lsq_scan.hpp) and radix sort (csrc/lsq_sort.hpp) alone, through lsq_debug_scan /
lsq_debug_sort, against the references of prims_ref.py -- at every size where the code takes another path: a lane's 16
values, a wave, a block or tile of 4 096, the 1 024 block sums (4 194 304 values) the scan's spine takes a round, and a
third round, where the carry is carried twice.  Then two of the tools above them across that round edge.  Every
comparison is exact."""
import numpy as np
import pytest

import lesseq_amd as L
from lesseq_amd import diffsplice as ds
from prims_ref import scan_ref, sort_ref, digits_ref, digit

pytestmark = pytest.mark.gpu

BLOCK = 4096                 # SCAN_BLOCK, SORT_TILE
ROUND = BLOCK * 1024         # values behind the block sums of one round of lsq_scan_spine_kernel

# form of lsq_debug_scan -> (pad, flag, dtype of the input); the pads are P2_GROUP_PAD / P1_GROUP_PAD of csrc/lsq_device.hpp
SCAN_FORMS = {"u32": (1, False, np.uint32), "flag": (1, True, np.uint32), "u64": (1, False, np.uint64),
              "pad_p2": (4, False, np.uint32), "pad_p1": (8, False, np.uint32)}
SMALL_N = [0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK + 1]
PAD_N = SMALL_N + [3 * BLOCK + 1]
LARGE_N = [BLOCK * 1023 + 1, ROUND - 1, ROUND, ROUND + 1, 2 * ROUND + 5]


def scan_patterns(form, n):
    """(name, values) of every pattern for one form and size"""
    pad, flag, dt = SCAN_FORMS[form]
    rng = np.random.default_rng(n * 8 + list(SCAN_FORMS).index(form))
    big = {"u32": 0xFFFFFFFF, "flag": 0xFFFFFFFF, "u64": (1 << 40) + 1, "pad_p2": 1000, "pad_p1": 1000}[form]
    yield "ones", np.ones(n, dtype=dt)
    yield "zeros", np.zeros(n, dtype=dt)
    yield "random", rng.integers(0, 1 << 16, n).astype(dt)
    # one nonzero value at the last index of a round (of a block, of the input, where the input ends sooner), and one at the
    # first index of the next
    last = ROUND - 1 if n >= ROUND else BLOCK - 1 if n >= BLOCK else n - 1
    first = ROUND if n > ROUND else BLOCK if n > BLOCK else 0
    for name, at in (("one_value_ending_a_round", last), ("one_value_beginning_a_round", first)):
        if 0 <= at < n:
            v = np.zeros(n, dtype=dt)
            v[at] = big
            yield name, v
    if pad > 1:
        yield "around_the_pad", rng.choice(np.array([0, 1, pad - 1, pad, pad + 1, 2 * pad - 1, 1000], dtype=dt), n)
    if flag:
        yield "flag_values", rng.choice(np.array([0, 1, 2, 0xFFFFFFFF], dtype=dt), n)


def check_scan(ctx, form, name, v):
    pad, flag, dt = SCAN_FORMS[form]
    assert v.dtype == dt
    got = ctx.debug_scan(form, v)
    want = np.arange(len(v) + 1, dtype=np.uint64) if name == "ones" and pad == 1 else scan_ref(v, pad, flag)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError("%s scan of %d values (%s): %d wrong, the first out[%d] = %d, expected %d"
                             % (form, len(v), name, len(bad), bad[0], got[bad[0]], want[bad[0]]))


@pytest.mark.parametrize("form", list(SCAN_FORMS))
def test_scan_up_to_a_few_blocks(gpu_ctx, form):
    for n in (PAD_N if SCAN_FORMS[form][0] > 1 else SMALL_N):
        for name, v in scan_patterns(form, n):
            check_scan(gpu_ctx, form, name, v)


@pytest.mark.parametrize("n", LARGE_N)
@pytest.mark.parametrize("form", ["u32", "flag", "u64"])
def test_scan_across_the_rounds_of_the_spine(gpu_ctx, form, n):
    for name, v in scan_patterns(form, n):
        check_scan(gpu_ctx, form, name, v)


def test_scan_of_ones_is_the_index(gpu_ctx):
    """prims_ref is not consulted: out[i] == i, on both sides of the second and of the third round"""
    n = 2 * ROUND + 5
    for form in ("u32", "flag", "u64"):
        got = gpu_ctx.debug_scan(form, np.ones(n, dtype=SCAN_FORMS[form][2]))
        assert np.array_equal(got, np.arange(n + 1, dtype=np.uint64)), form


@pytest.mark.parametrize("n", [65, BLOCK + 1, 2 * BLOCK + 1, ROUND + 1])
def test_scan_u64_carries_across_bit_32(gpu_ctx, n):
    """2^32 - 1 in every lane: the two halves scan_wave_incl shuffles apart carry into each other between lanes, waves and blocks"""
    v = np.full(n, 0xFFFFFFFF, dtype=np.uint64)
    got = gpu_ctx.debug_scan("u64", v)
    assert np.array_equal(got, np.arange(n + 1, dtype=np.uint64) * np.uint64(0xFFFFFFFF))
    assert np.array_equal(got, scan_ref(v))


def test_scan_u64_of_values_below_2_40(gpu_ctx):
    v = np.random.default_rng(40).integers(0, 1 << 40, (1 << 20) + 1, dtype=np.uint64)
    check_scan(gpu_ctx, "u64", "below_2_40", v)


@pytest.mark.parametrize("n", [2, 65, BLOCK + 1, 2 * BLOCK + 1])
def test_scan_u64_with_a_total_just_below_2_64(gpu_ctx, n):
    """one value of 2^63, then small ones: the total stays below 2^64, as lsq_scan.hpp asks of its callers"""
    v = np.random.default_rng(n).integers(0, 1 << 40, n, dtype=np.uint64)
    v[0] = 1 << 63
    check_scan(gpu_ctx, "u64", "2_63_first", v)
    v[0], v[n // 2] = v[n // 2], v[0]
    check_scan(gpu_ctx, "u64", "2_63_in_the_middle", v)


def test_scan_rejects_an_unknown_form(gpu_ctx):
    for form in (-1, 5):
        with pytest.raises(L.LsqError) as e:
            gpu_ctx.debug_scan(form, np.ones(3, dtype=np.uint32))
        assert e.value.status == -1          # LSQ_E_ARG


# ---- the sort -----------------------------------------------------------------------------------------------------------

# name -> (the digits, (word, shift) of 32 bits that no digit names: the tests keep the input index there)
DIGIT_LISTS = {
    "adjust_8": ([0, 8, 16, 24, 32, 40, 48, 56], (1, 0)),                          # all of w0 (lsq_as_adjust)
    "junctions_10": ([0, 8, 16, 24, 32, 40, 48, 56, 64 + 32, 64 + 40], (1, 0)),     # lsq_junc.hip
    "both_words_5": ([8, 24, 64, 72, 112], (0, 32)),                               # digits and payload in both words
    "single_1": ([40], (1, 0)),
    "descending_2": ([16, 0], (1, 16)),                                            # the digit at bit 0 is the primary key
    "unaligned_3": ([4, 100, 52], (0, 12)),                                        # digits at no byte's edge; bits 12 .. 43 of w0 are free
}
SORT_SMALL_N = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 1000]
SORT_PATTERNS = ["random", "sorted", "reversed", "equal", "alternating", "period_256", "period_257", "tile_but_last_above", "tile_but_last_below", "ties"]


def compose(n, bits, field, digits, rng):
    """records whose digit at bits[j] is digits[j] (uint8 arrays; None: random), with the input index in the 32 bits at
    `field` and random bits everywhere else"""
    w = [rng.integers(0, 1 << 64, n, dtype=np.uint64), rng.integers(0, 1 << 64, n, dtype=np.uint64)]
    for b, d in zip(bits, digits):
        if d is not None:
            k, sh = b >> 6, np.uint64(b & 63)
            w[k] = (w[k] & ~(np.uint64(0xFF) << sh)) | (d.astype(np.uint64) << sh)
    k, sh = field[0], np.uint64(field[1])
    w[k] = (w[k] & ~(np.uint64(0xFFFFFFFF) << sh)) | (np.arange(n, dtype=np.uint64) << sh)
    return w[0], w[1]


def sort_input(pattern, n, bits, field):
    rng = np.random.default_rng(n * 16 + SORT_PATTERNS.index(pattern))
    i = np.arange(n, dtype=np.uint64)
    nd = len(bits)

    def of_rank(r):      # byte j of a 64-bit rank as the digit j of the list (the list's digits past the eighth: zero)
        return [((r >> np.uint64(8 * j)) & np.uint64(0xFF)).astype(np.uint8) if j < 8 else np.zeros(n, dtype=np.uint8) for j in range(nd)]

    if pattern == "random":
        d = [None] * nd
    elif pattern in ("sorted", "reversed"):
        r = np.sort(rng.integers(0, 1 << (8 * min(nd, 8)), n, dtype=np.uint64))
        d = of_rank(r if pattern == "sorted" else r[::-1].copy())
    elif pattern == "equal":
        d = [np.full(n, 0x5A + j, dtype=np.uint8) for j in range(nd)]
    elif pattern == "alternating":          # two values, lane by lane
        d = [np.where(i & np.uint64(1), 0xC3 - j, 0x3C + j).astype(np.uint8) for j in range(nd)]
    elif pattern in ("period_256", "period_257"):
        p = np.uint64(int(pattern[-3:]))
        d = [(((i + np.uint64(j)) % p) & np.uint64(0xFF)).astype(np.uint8) for j in range(nd)]
    elif pattern in ("tile_but_last_above", "tile_but_last_below"):      # a tile's records in one digit value, except its last
        odd = 200 if pattern.endswith("above") else 3
        d = [np.where(i % np.uint64(BLOCK) == np.uint64(BLOCK - 1), odd, 7).astype(np.uint8) for j in range(nd)]
    else:                                   # "ties": three values of the least significant digit, the others constant
        d = [rng.integers(0, 3, n).astype(np.uint8)] + [np.full(n, 9, dtype=np.uint8) for j in range(1, nd)]
    return compose(n, bits, field, d, rng)


def assert_stable(w0, w1, bits, field):
    """within every run of records equal on the sorted digits the input index ascends"""
    if len(w0) < 2:
        return
    same = np.ones(len(w0) - 1, dtype=bool)
    for b in bits:
        d = digit(w0, w1, b)
        same &= d[1:] == d[:-1]
    idx = ((w0, w1)[field[0]] >> np.uint64(field[1])) & np.uint64(0xFFFFFFFF)
    assert np.all(idx[1:][same] > idx[:-1][same])


def check_sort(ctx, w0, w1, bits, field, what):
    r0, r1 = sort_ref(w0, w1, bits)
    kept = digits_ref(w0, w1, bits)
    for drop in (False, True):
        g0, g1, n_passes = ctx.debug_sort(w0, w1, bits, drop_constant=drop)
        assert np.array_equal(g0, r0) and np.array_equal(g1, r1), (what, drop)
        assert n_passes == (len(kept) if drop else len(bits) if len(w0) > 1 else 0), (what, drop)
    assert_stable(g0, g1, bits, field)
    return g0, g1


@pytest.mark.parametrize("name", list(DIGIT_LISTS))
def test_sort_every_pattern_up_to_a_few_tiles(gpu_ctx, name):
    bits, field = DIGIT_LISTS[name]
    for n in SORT_SMALL_N:
        for pattern in SORT_PATTERNS:
            w0, w1 = sort_input(pattern, n, bits, field)
            check_sort(gpu_ctx, w0, w1, bits, field, (name, n, pattern))


@pytest.mark.parametrize("name", list(DIGIT_LISTS))
def test_sort_with_a_digit_table_of_several_scan_blocks(gpu_ctx, name):
    """65 537 records: 17 tiles, a digit table of 4 352 counters (more than one scan block)"""
    bits, field = DIGIT_LISTS[name]
    for pattern in SORT_PATTERNS:
        w0, w1 = sort_input(pattern, 65537, bits, field)
        check_sort(gpu_ctx, w0, w1, bits, field, (name, pattern))


@pytest.mark.parametrize("name", list(DIGIT_LISTS))
def test_sort_of_a_million_records(gpu_ctx, name):
    """1 048 577 records: 257 tiles, a digit table of 65 792 counters (17 scan blocks)"""
    bits, field = DIGIT_LISTS[name]
    for pattern in SORT_PATTERNS:
        w0, w1 = sort_input(pattern, (1 << 20) + 1, bits, field)
        check_sort(gpu_ctx, w0, w1, bits, field, (name, pattern))


@pytest.mark.parametrize("n", SORT_SMALL_N + [65537, (1 << 20) + 1])
def test_sort_by_all_of_w0_gives_the_stable_argsort(gpu_ctx, n):
    """lsq_as_adjust's use: the eight digits of w0, the index in w1 -- doubles with ties as keys"""
    rng = np.random.default_rng(n)
    p = rng.uniform(size=n) ** 3
    if n > 4:
        p[rng.integers(0, n, n // 4)] = p[rng.integers(0, n, n // 4)]
        p[rng.integers(0, n, n // 20 + 1)] = 0.0
        p[rng.integers(0, n, n // 20 + 1)] = 1.0
    w0 = p.view(np.uint64)
    g0, g1, n_passes = gpu_ctx.debug_sort(w0, np.arange(n, dtype=np.uint64), DIGIT_LISTS["adjust_8"][0])
    order = np.argsort(w0, kind="stable")
    assert np.array_equal(g1, order.astype(np.uint64)) and np.array_equal(g0, w0[order])
    assert n_passes == (8 if n > 1 else 0)


def test_sort_all_equal_records_come_back_untouched(gpu_ctx):
    for name, (bits, field) in DIGIT_LISTS.items():
        for n in (2, 1025, 2 * BLOCK + 1):
            w0, w1 = sort_input("equal", n, bits, field)
            for drop, passes in ((False, len(bits)), (True, 0)):
                g0, g1, n_passes = gpu_ctx.debug_sort(w0, w1, bits, drop_constant=drop)
                assert np.array_equal(g0, w0) and np.array_equal(g1, w1) and n_passes == passes, (name, n, drop)


def test_sort_twice_gives_the_same(gpu_ctx):
    for name, (bits, field) in DIGIT_LISTS.items():
        for pattern in ("random", "ties"):
            w0, w1 = sort_input(pattern, 3 * BLOCK + 1000, bits, field)
            a, b = gpu_ctx.debug_sort(w0, w1, bits), gpu_ctx.debug_sort(w0, w1, bits)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2], (name, pattern)


def test_sort_rejects_digits_out_of_range(gpu_ctx):
    w = np.arange(4, dtype=np.uint64)
    for bits in ([121], [0, 128], [0, 8] * 8 + [16]):         # past the last digit of w1; 17 digits
        with pytest.raises(L.LsqError) as e:
            gpu_ctx.debug_sort(w, w, bits)
        assert e.value.status == -1          # LSQ_E_ARG
    assert np.array_equal(gpu_ctx.debug_sort(w[::-1], w, [120, 60])[0], w[::-1])       # the last digit of each word: all zero here


# ---- the tools above them, across the spine's round edge ----------------------------------------------------------------

@pytest.mark.parametrize("n", [ROUND + 1, 2 * ROUND + 7])
def test_adjust_across_the_spine_round(gpu_ctx, n):
    """lsq_as_adjust: the flag scan over n values and the compaction behind it, with NaNs on both sides of value 4 194 304"""
    from test_as_gpu import adjust_ref
    rng = np.random.default_rng(n)
    p = rng.uniform(size=n) ** 3
    p[rng.integers(0, n, n // 20)] = p[rng.integers(0, n, n // 20)]          # ties
    p[::1000] = np.nan
    p[ROUND - 70:ROUND - 3] = np.nan
    p[ROUND + 2:ROUND + 45] = np.nan
    if n > 2 * ROUND:
        p[2 * ROUND - 33:2 * ROUND - 1] = np.nan
        p[2 * ROUND + 1:2 * ROUND + 5] = np.nan
    bon, bh = ds.adjust(gpu_ctx, p)
    rb, rh = adjust_ref(p)
    assert bon.tobytes() == rb.tobytes()
    assert bh.tobytes() == rh.tobytes()


def test_mrf_lines_across_the_spine_round(tmp_path):
    """An MRF text of 4 096 * 1 024 + 9 reads: the scans over its lines take a second round of the spine.  A few two-block
    lines before and after line 4 194 304, so that block offsets past the carry differ from line numbers."""
    from test_mrf_device import setup, write_annot, parsed_equal
    iv, mp = write_annot(tmp_path)
    one, two = b"c1:+:101:150:1:50\n", b"c1:+:101:150:1:50,c1:+:301:350:51:100\n"
    n = ROUND + 9
    doubled = [5, BLOCK - 1, ROUND - BLOCK, ROUND - 2, ROUND - 1, ROUND, ROUND + 1, ROUND + 7, n - 1]       # (data lines, from 0)
    parts, at = [b"AlignmentBlocks\n"], 0
    for k in doubled:
        parts += [one * (k - at), two]
        at = k + 1
    parts.append(one * (n - at))
    p = tmp_path / "round.mrf"
    p.write_bytes(b"".join(parts))
    ev, ctx = setup(iv, mp)
    host, dev = L.Reads.from_mrf(str(p), ev), ctx.parse_mrf_device(str(p))
    assert len(host) == n and host.num_blocks == n + len(doubled)
    parsed_equal(ev, host, dev)
    off = host.arrays()[0]
    assert int(off[ROUND]) == ROUND + 5 and int(off[n]) == n + len(doubled)      # (the offsets past the carry are not the line numbers)
    ctx.close()
