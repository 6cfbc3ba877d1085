"""The read bootstrap's resampling on the host: the generator's known answers through the Python reference of
tests/bootstrap_ref.py, then lsq_bootstrap_resample_host -- the code the device runs, csrc/lsq_philox.hpp -- against that
reference, exactly.  No GPU."""
import numpy as np
import pytest

import lesseq_amd as L
import bootstrap_ref as B

SEEDS = (0, 0x9E3779B97F4A7C15)
REPLICATES = (0, 1, 4095)

KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter, key, want", KNOWN)
def test_known_answers_of_the_generator(counter, key, want):
    got = B.philox4x32_10(counter, key)
    assert tuple(int(x[0]) for x in got) == want


def test_reference_arithmetic():
    """the reference's own pieces: an array of counters gives each counter's block; the high multiply by limbs"""
    j = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 5], np.uint64)
    got = B.philox4x32_10((j & B.MASK32, j >> np.uint64(32), 7, 9), (3, 4))
    for i, v in enumerate(j.tolist()):
        one = B.philox4x32_10((v & 0xFFFFFFFF, v >> 32, 7, 9), (3, 4))
        assert [int(x[i]) for x in got] == [int(x[0]) for x in one]
    assert len({tuple(int(x[i]) for x in got) for i in range(len(j))}) == len(j)
    assert int(B.mul_hi(np.array([2 ** 64 - 1], np.uint64), 2 ** 64 - 1)[0]) == 2 ** 64 - 2
    assert int(B.mul_hi(np.array([2 ** 63], np.uint64), 7)[0]) == 3


# one event per case: counts[m][class - 1]
CASES = {
    "n0_K2": [[0, 0, 0]],
    "n1_K2": [[0, 1, 0]],
    "n2_K2": [[1, 0, 1]],                     # one block, both halves
    "n3_K2": [[1, 1, 1]],                     # the last block half used
    "gap_K2": [[5, 0, 9]],                    # a class without reads between two with: the search skips it
    "last_K2": [[0, 0, 40]],                  # every read in the last class
    "n0_K3": [[0] * 7],
    "n1_K3": [[0, 0, 0, 1, 0, 0, 0]],
    "n3_K3": [[0, 2, 0, 0, 0, 1, 0]],
    "gaps_K3": [[3, 0, 0, 8, 0, 1, 0]],
    "last_K3": [[0, 0, 0, 0, 0, 0, 25]],
    "two_files_K2": [[4, 0, 3], [0, 0, 2]],
    "two_files_K3": [[1, 0, 2, 0, 3, 0, 4], [0, 0, 0, 0, 0, 0, 0]],
    "two_files_n1": [[0, 0, 0], [1, 0, 0]],
    "thousand_K2": [[300, 0, 700]],
    "thousand_K3_two": [[100, 200, 0, 300, 0, 0, 400], [0, 500, 0, 0, 500, 0, 0]],
}


def one_event(rows):
    cnt = np.array(rows, np.uint64)
    return np.array([0, cnt.shape[1]], np.uint64), cnt


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_resampling_is_the_reference(name):
    off, cnt = one_event(CASES[name])
    for seed in SEEDS:
        for b in REPLICATES:
            got = L.bootstrap_resample_host(off, cnt, seed, b)
            want = B.resample(off, cnt, seed, b)
            assert got.dtype == np.uint64 and np.array_equal(got, want), (name, seed, b, got, want)
            assert np.array_equal(got.sum(axis=1), cnt.sum(axis=1))                 # a pair keeps its total
            assert not got[cnt == 0].any()                                           # a class without reads draws none


def test_event_number_and_read_file_enter_the_counter():
    """several events in one call: event e of read file m draws with (e, m) in the counter, whatever lies around it"""
    rows = [CASES["thousand_K2"][0] + CASES["n0_K2"][0] + CASES["gaps_K3"][0] + CASES["thousand_K2"][0],
            CASES["thousand_K2"][0] + CASES["n3_K2"][0] + CASES["last_K3"][0] + CASES["thousand_K2"][0]]
    off = np.array([0, 3, 6, 13, 16], np.uint64)
    cnt = np.array(rows, np.uint64)
    got = L.bootstrap_resample_host(off, cnt, 5, 2)
    assert np.array_equal(got, B.resample(off, cnt, 5, 2))
    # the same counts as event 0 and as event 3, as read file 0 and as read file 1: four different replicates
    four = {tuple(got[m, a:a + 3]) for m in (0, 1) for a in (0, 13)}
    assert len(four) == 4, four
    for m in (0, 1):
        for e in range(4):
            assert got[m, int(off[e]):int(off[e + 1])].sum() == cnt[m, int(off[e]):int(off[e + 1])].sum()


@pytest.mark.parametrize("n", [2 ** 32 + 3, 2 ** 40])
def test_high_multiply_above_32_bits(n):
    """n beyond 32 bits over three classes: the first 1000 draws, and 1000 around draw 2^32 (the block counter's high word)"""
    counts = [n // 3, n // 2 - n // 3, n - n // 2]
    for seed in SEEDS:
        for b in (0, 4095):
            got = L.bootstrap_draws(counts, seed, 1, 77, b, 0, 1000)
            want = B.draws(counts, seed, 1, 77, b, 0, 1000)
            assert np.array_equal(got, want)
            assert set(got.tolist()) == {1, 2, 3}
            first = 2 ** 33 - 499 if n > 2 ** 34 else n - 1000
            assert np.array_equal(L.bootstrap_draws(counts, seed, 1, 77, b, first, 1000), B.draws(counts, seed, 1, 77, b, first, 1000))
    with pytest.raises(L.LsqError) as ei:
        L.bootstrap_draws(counts, 0, 0, 0, 0, n - 1, 2)
    assert ei.value.status == -5


def test_replicates_and_seeds_differ_and_repeat():
    off, cnt = one_event(CASES["thousand_K3_two"])
    base = L.bootstrap_resample_host(off, cnt, 11, 3)
    assert np.array_equal(base, L.bootstrap_resample_host(off, cnt, 11, 3))
    assert not np.array_equal(base, L.bootstrap_resample_host(off, cnt, 11, 4))
    assert not np.array_equal(base, L.bootstrap_resample_host(off, cnt, 12, 3))
    assert not np.array_equal(base, L.bootstrap_resample_host(off, cnt, 11 + 2 ** 32, 3))       # the seed's high word is in the key
    assert not np.array_equal(base[0], cnt[0]) and base[0].sum() == 1000 and base[1].sum() == 1000


def test_bad_arguments():
    off, cnt = one_event(CASES["n3_K2"])
    for b in (2 ** 24, 2 ** 32 - 1):
        with pytest.raises(L.LsqError) as ei:
            L.bootstrap_resample_host(off, cnt, 0, b)
        assert ei.value.status == -1
    assert L.lib.lsq_bootstrap_tile() >= 2 and L.lib.lsq_bootstrap_tile() % 2 == 0
