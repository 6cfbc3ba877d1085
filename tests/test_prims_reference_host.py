"""The references of tests/prims_ref.py against brute force in Python integers, on inputs small enough to loop over: what
the device primitives are compared with (tests/test_prims_direct_gpu.py) is itself held to the definitions here."""
import numpy as np
import pytest

from prims_ref import scan_ref, sort_ref, digits_ref

# (pad, flag, bits of an input value) of the five forms the library instantiates (include/lesseq_hip_dev.h, lsq_debug_scan)
FORMS = [(1, False, 32), (1, True, 32), (1, False, 64), (4, False, 32), (8, False, 32)]


def scan_loop(values, pad, flag):
    out, run = [0], 0
    for v in values:
        v = int(v)
        run += (1 if v else 0) if flag else (v + pad - 1) // pad * pad
        out.append(run)
    return out


@pytest.mark.parametrize("pad,flag,width", FORMS)
def test_scan_ref_equals_a_loop_over_python_integers(pad, flag, width):
    rng = np.random.default_rng(pad * 10 + flag + width)
    dt = np.uint32 if width == 32 else np.uint64
    edges = [0, 1, pad - 1, pad, pad + 1, 2 ** 32 - pad]
    if width == 64:
        edges += [2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3]
    v = np.concatenate([np.array(edges, dtype=dt), rng.integers(0, 1 << 16, 300).astype(dt), np.array(edges[::-1], dtype=dt)])
    rng.shuffle(v)
    got = scan_ref(v, pad, flag)
    assert got.dtype == np.uint64 and len(got) == len(v) + 1
    assert [int(x) for x in got] == scan_loop(v, pad, flag)
    # the empty input and a single value
    assert [int(x) for x in scan_ref(np.zeros(0, dtype=dt), pad, flag)] == [0]
    assert [int(x) for x in scan_ref(np.array([2 ** 32 - pad], dtype=dt), pad, flag)] == scan_loop([2 ** 32 - pad], pad, flag)


def test_scan_ref_holds_sums_past_32_and_up_to_64_bits():
    v = np.full(70, 2 ** 32 - 1, dtype=np.uint64)
    assert [int(x) for x in scan_ref(v)] == [i * (2 ** 32 - 1) for i in range(71)]
    v = np.array([2 ** 63, 5, 0, 2 ** 62], dtype=np.uint64)
    assert [int(x) for x in scan_ref(v)] == [0, 2 ** 63, 2 ** 63 + 5, 2 ** 63 + 5, 2 ** 63 + 2 ** 62 + 5]


def digit_of(a, b, bit):
    return ((a >> bit) if bit < 64 else (b >> (bit - 64))) & 0xFF


def sort_loop(w0, w1, bits):
    recs = [(int(a), int(b)) for a, b in zip(w0, w1)]
    order = sorted(range(len(recs)), key=lambda i: tuple(digit_of(recs[i][0], recs[i][1], bit) for bit in reversed(bits)) + (i,))
    return [recs[i][0] for i in order], [recs[i][1] for i in order]


@pytest.mark.parametrize("bits", [[0, 8, 16, 24, 32, 40, 48, 56], [0, 8, 16, 24, 32, 40, 48, 56, 96, 104], [8, 24, 64, 72, 112], [40], [16, 0], [120], [60], []])
def test_sort_ref_equals_sorted_with_the_input_index_as_tie_break(bits):
    rng = np.random.default_rng(len(bits))
    n = 400
    full = rng.integers(0, 1 << 64, n, dtype=np.uint64), rng.integers(0, 1 << 64, n, dtype=np.uint64)
    # few distinct values per digit, so that most records tie on most digits and the order of equals is what is tested
    mask = np.uint64(0x0303030303030303)
    few = full[0] & mask, full[1] & mask
    for w0, w1 in (full, few, (full[0][:1], full[1][:1]), (full[0][:0], full[1][:0])):
        g0, g1 = sort_ref(w0, w1, bits)
        e0, e1 = sort_loop(w0, w1, bits)
        assert [int(x) for x in g0] == e0 and [int(x) for x in g1] == e1
        assert g0.dtype == np.uint64 and g1.dtype == np.uint64


def test_sort_ref_follows_the_list_not_the_bit_positions():
    w0 = np.array([0x010002, 0x020001, 0x010001, 0x020002], dtype=np.uint64)      # digit at bit 16 | digit at bit 0
    w1 = np.arange(4, dtype=np.uint64)
    assert [int(x) for x in sort_ref(w0, w1, [0, 16])[1]] == [2, 0, 1, 3]           # bit 16 the primary key
    assert [int(x) for x in sort_ref(w0, w1, [16, 0])[1]] == [2, 1, 0, 3]           # bit 0 the primary key
    assert [int(x) for x in sort_ref(w0, w1, [16])[1]] == [0, 2, 1, 3]              # ties keep the input's order


def test_digits_ref_on_hand_made_cases():
    z = np.zeros(3, dtype=np.uint64)
    assert digits_ref(z, z, [0, 8, 64]) == []
    assert digits_ref(z[:0], z[:0], [0, 8]) == [] and digits_ref(z[:1] + np.uint64(77), z[:1], [0, 8]) == []
    w0 = np.array([0x00FF00, 0x00FE00, 0x00FF00], dtype=np.uint64)
    w1 = np.array([1 << 40, 1 << 40, 1 << 47], dtype=np.uint64)
    assert digits_ref(w0, w1, [0, 8, 16, 64 + 32, 64 + 40]) == [8, 64 + 40]
    assert digits_ref(w0, w1, [64 + 40, 8, 0]) == [64 + 40, 8]                      # in the order given
    assert digits_ref(w0, w1, [4]) == [4] and digits_ref(w0, w1, [12]) == [] and digits_ref(w0, w1, [1]) == [1]      # a digit at any bit position
    # records that differ only in bits no digit names
    assert digits_ref(np.array([1 << 20, 1 << 21], dtype=np.uint64), z[:2], [0, 8, 24]) == []
