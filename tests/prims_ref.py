"""References for the two device primitives (csrc/lsq_scan.hpp, csrc/lsq_sort.hpp), written from their definitions and
not from the kernels: no blocks, tiles, waves or carries in here.  tests/test_prims_reference_host.py holds them against
brute force on small inputs; tests/test_prims_direct_gpu.py holds the kernels against them."""
import numpy as np


def scan_ref(values, pad=1, flag=False):
    """out[i] = sum of f(values[:i]) in uint64, out[n] the total: f rounds up to a multiple of `pad` (a power of two), or,
    with `flag`, maps to 0 / 1.  f is applied in uint64, so a 32-bit value within `pad` of 2^32 does not wrap here (the
    device's 32-bit padded forms do; no caller has such values, and no test feeds them)."""
    v = np.asarray(values).astype(np.uint64)
    if flag:
        f = (v != 0).astype(np.uint64)
    else:
        f = (v + np.uint64(pad - 1)) & ~np.uint64(pad - 1)
    out = np.zeros(len(v) + 1, dtype=np.uint64)
    np.cumsum(f, dtype=np.uint64, out=out[1:])
    return out


def digit(w0, w1, bit):
    """the 8-bit digit that begins at `bit` of the 128 bits w1:w0 (a digit does not run on from w0 into w1)"""
    w = np.asarray(w0 if bit < 64 else w1, dtype=np.uint64)
    return ((w >> np.uint64(bit & 63)) & np.uint64(0xFF)).astype(np.uint8)


def sort_ref(w0, w1, bits):
    """the records in stable order by the digits at `bits`, least significant first as listed; bits that no digit names
    come along unchanged beside their record.  Returns the permuted pair."""
    w0, w1 = np.asarray(w0, dtype=np.uint64), np.asarray(w1, dtype=np.uint64)
    if len(bits) == 0 or len(w0) == 0:
        return w0.copy(), w1.copy()
    order = np.lexsort([digit(w0, w1, b) for b in bits])        # stable; its last key is the primary one
    return w0[order], w1[order]


def digits_ref(w0, w1, bits):
    """the subset of `bits` on which the records differ, in order"""
    out = []
    for b in bits:
        d = digit(w0, w1, b)
        if len(d) and d.min() != d.max():
            out.append(b)
    return out
