"""Compact pool records that keep a block's END (csrc/lsq_device.hpp COMPACT_*: end << 10 | length) and are compared in
place by the count kernel's streaming loops (csrc/lsq_count.hip: stream_pool1_compact, stream_pool2_compact).

What the format adds to what tests/test_count_paths_gpu.py and tests/test_parity_gpu.py already hold:
  * a record is compared as a whole word with a threshold word (end << 10 | 0x3FF): reads that end one before, on and one
    behind every segment end of one- and two-owner cells, with the lengths 1, 2, 100 and 1 023 (the longest a record holds);
  * the padding of a cell's group and of a junction group is no longer an empty read the loops test for, but a value the
    compares pass over and a count the lane takes from its last record: cells of 1 to 17 reads and junction groups of 1 to 9,
    so that every number of padding records occurs in a last group;
  * a block must END within 22 bits: block ends and second-block reaches on both sides of that edge, in a bucket of more than
    2 Mi bases;
  * the replay reads the pools back through the same unpack helper;
  * pack and unpack on the host, through lsq_debug_compact_record.
Expectations are the oracle's rows (oracle_binding) and the host's compact_block_fits; every file is counted under wide
records and under both compact kernels, by the release library here and by the developer library in a child process
(count_paths_child.py) on grids of one and of three workgroups."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import lesseq_amd as L
import oracle_binding as ob
import count_paths_inputs as ci

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_LIB = os.path.join(ROOT, "lesseq_amd", "_build", "liblesseq_hip_dev.so")
CHILD = os.path.join(ROOT, "tests", "count_paths_child.py")
CHILD_TIMEOUT = 120
OPTIONS = {"wide": {"compact_pools": 0}, "compact4": {"reads_per_look": 4}, "compact8": {"reads_per_look": 8}}
KERNELS = tuple(OPTIONS)
COUNTERS_ON = 256               # LSQ_ABLATE of the developer library: path counters, results untouched
END_MAX = (1 << 22) - 2         # the farthest end of a block in a compact record (COMPACT_END_MAX)
PAD = ((1 << 22) - 1) << 10     # COMPACT_PAD: at and above it a word of the one-block pool is padding
BIAS = 1 << 21                  # COMPACT_BIAS

# P: two forms that split its first exon into the abutting segments [10000,11100) [11100,11300); Q lies over both (two-owner
# cells from 10500 on); R covers the bases behind P's first exon, so that a read may end one base past it
PQR = [("P", "+", [[(10000, 11300), (12000, 12100)], [(10000, 11100), (12000, 12100)]]),
       ("Q", "+", [[(10500, 11200), (12500, 12600)], [(10500, 11200)]]),
       ("R", "-", [[(11250, 11400), (11600, 11700)], [(11250, 11400)]])]
PQR_ENDS = (11100, 11200, 11300)
# G: one gene whose introns are longer than 2 Mi and 4 Mi bases -- one bucket, first base 1000
G_LO = 1000
G_EX = [(G_LO, G_LO + 400), (G_LO + BIAS - 300, G_LO + BIAS + 300), (G_LO + (1 << 22), G_LO + (1 << 22) + 500)]
GENE_G = [("G", "+", [[G_EX[0], G_EX[1], G_EX[2]], [G_EX[0], G_EX[2]]])]


def compact_record(which, off, length):
    """lsq_debug_compact_record: (fits, record, start, end)"""
    f = L.lib.lsq_debug_compact_record
    f.argtypes = [C.c_int, C.c_longlong, C.c_longlong, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    f.restype = C.c_int
    rec, s, e = C.c_uint32(0), C.c_int32(0), C.c_int32(0)
    rc = f(which, off, length, C.byref(rec), C.byref(s), C.byref(e))
    assert rc in (0, 1), (which, off, length, rc)
    return rc == 1, int(rec.value), int(s.value), int(e.value)


def fits(off, length):
    return compact_record(0, off, length)[0]


def test_pack_and_unpack_on_the_host():
    """all four corners of (offset, length) come back as they went in; a record orders blocks by their end; what does not
    fit is refused; no block gives a padding value, and padding unpacks to an empty block"""
    top = 0
    for length in (1, 1023):
        for off in (0, END_MAX - length):
            ok, rec, s, e = compact_record(0, off, length)
            assert ok and (s, e) == (off, off + length), (off, length, rec, s, e)
            assert rec == ((off + length) << 10 | length) and rec < PAD
            top = max(top, rec)
    assert top == (END_MAX << 10 | 1023) == PAD - 1          # the largest record of a block: just below the padding
    for off, length in ((END_MAX, 1), (END_MAX - 1022, 1023), (0, 1024), (0, 0), (-1, 5), (1 << 22, 1), ((1 << 22) - 1, 1)):
        assert not fits(off, length), (off, length)
    rng = np.random.default_rng(3)
    offs, lens = rng.integers(0, END_MAX - 1023, 400), rng.integers(1, 1024, 400)
    recs = [compact_record(0, int(o), int(n))[1] for o, n in zip(offs, lens)]
    for i in range(0, 400, 2):
        a, b = int(offs[i] + lens[i]), int(offs[i + 1] + lens[i + 1])
        if a != b:
            assert (a < b) == (recs[i] < recs[i + 1])
    for in_group in range(1, 8):
        for in_half in range(1, 5):
            ok, rec, s, e = compact_record(1, in_group, in_half)
            assert ok and rec >= PAD and s == e, (in_group, in_half, rec, s, e)
            assert rec & 15 == in_group and (rec >> 4) & 15 == in_half
            ok, rec, s, e = compact_record(2, in_group, in_half)
            # (block 1 of a two-block padding record: no bases, which no block has; its block 2 is 0)
            assert ok and rec & 0x3FF == 0 and s == e and rec >> 10 == (in_group | in_half << 4), (in_group, in_half, rec, s, e)


# ---- the files -------------------------------------------------------------------------------------------------------

def threshold_file(cov):
    """reads that end one before, on and one behind P's and Q's segment ends, 1 / 2 / 100 / 1 023 bases long (and two lengths
    between, which start in the two-owner cells); some of them twice, so that groups of the pool fill differently"""
    reads = []
    for t in PQR_ENDS:
        for d in (-1, 0, 1):
            for n in (1, 2, 100, 400, 700, 1023):
                rd = (t + d - n, t + d)
                if ci.loadable(cov, rd):
                    reads += [rd] * (2 if n in (2, 1023) else 1)
    # two-block reads over P's junction whose block 2 ends one before, on and one behind the segment's end
    for y, n1 in ((11300, 1), (11300, 100), (11300, 1023), (11100, 1), (11100, 1023)):
        for w in (12099, 12100):
            for z in (12000,):
                reads.append((y - n1, y, z, w))
    return reads


def padding_file(k):
    """k reads that start in P's one-owner cell (the ends on and about its thresholds), 18 - k in Q's last cell, junction
    groups of (k - 1) % 9 + 1 and 9 - (k - 1) % 9 two-block reads, and one to five two-block reads that cross no junction"""
    ends = (11100, 11300, 11099, 11101, 11299, 11301, 10490, 11100, 11300)
    reads = [(10400 + 5 * q, ends[q % len(ends)]) for q in range(k)]           # (no block longer than 1 023 bases: all fit compact records)
    reads += [(12510 + q, 12560 + q) for q in range(18 - k)]
    j = (k - 1) % 9 + 1
    reads += [(11200 + q, 11300, 12000, 12050 + 10 * (q % 5)) for q in range(j)]           # long form of P: 11300 | 12000
    reads += [(10300 + q, 11100, 12000, 12100 - (q % 3)) for q in range(10 - j)]           # short form: 11100 | 12000
    # ... and a group that crosses no junction of its own: block 1 starts in a cell of two owners
    reads += [(10600 + q, 11100, 12000, 12100 - (q % 3)) for q in range(plain_group(k))]
    return reads


def plain_group(k):
    return (3 * k) % 5 + 1


def cut_file():
    """one cell of 24 reads and nothing else: three whole groups of eight, for a grid of three workgroups to cut between"""
    return [(10200 + q, 11100 + (q % 3) - 1) for q in range(24)]


def edge_file():
    """block ends 2^22 - 2 .. 2^22 + 1 in a record's terms (the bucket's first base - 2^21 is 0), as one-block reads, as block
    1 of two-block reads, and as the reach of a second block; among reads enough that the file stays compact"""
    reads = [(G_LO + 3 * (q % 90), G_LO + 3 * (q % 90) + 100) for q in range(700)]
    reads += [(G_LO + 50 + q % 40, G_EX[0][1], G_EX[1][0], G_EX[1][0] + 80 + q % 7) for q in range(60)]
    for d in (-2, -1, 0, 1):
        e = G_LO - BIAS + (1 << 22) + d                  # the end whose offset is 2^22 + d
        for n in (1, 50, 100):
            reads.append((e - n, e))
        reads.append((e - 60, e, G_EX[2][0], G_EX[2][0] + 40))
        y = G_LO + 200
        w = y + (1 << 22) + d                            # block 2 ends 2^22 + d behind block 1
        reads.append((y - 100, y, w - 50, w))
    return reads


def expected_pools(reads, lo):
    """(one-block, two-block, third-pool) reads as compact_block_fits sorts them on the host"""
    n = [0, 0, 0]
    for rd in reads:
        ok = fits(rd[0] - lo + BIAS, rd[1] - rd[0])
        if len(rd) == 4:
            ok = ok and fits(rd[2] - rd[1], rd[3] - rd[2])
        n[(0 if len(rd) == 2 else 1) if ok else 2] += 1
    return tuple(n)


def table(ev, cnt, bases):
    """per gene: support, matched bases, reads per isoform -- the rows the oracle gives"""
    cnt, bases = np.asarray(cnt, np.int64), np.asarray(bases, np.int64)
    off = ev.class_offsets()
    out = []
    for i in range(len(ev)):
        K = ev.K(i)
        cl = cnt[off[i]:off[i + 1]]
        out += [int(cl.sum()), int(bases[off[i]:off[i + 1]].sum())] + [int(sum(cl[c - 1] for c in range(1, 1 << K) if c >> j & 1)) for j in range(K)]
    return np.array(out, np.int64)


class World:
    def __init__(self, d):
        self.d = str(d)
        self.ann = {}
        for stem, genes in (("pqr", PQR), ("g", GENE_G)):
            iv, mp = ci.write_annotation(self.d, stem, genes)
            ev = L.Events(L.Annotation(iv, mp), ("SHORT_READ",), (100,))
            self.ann[stem] = dict(interval=iv, map=mp, cov=ev.covered(ci.CHROM), ev=ev)
        assert self.ann["g"]["ev"].num_buckets == 1
        files = [("thresholds", "pqr", threshold_file(self.ann["pqr"]["cov"]))]
        files += [("pad%02d" % k, "pqr", padding_file(k)) for k in range(1, 18)]
        files += [("cut", "pqr", cut_file()), ("edge22", "g", edge_file())]
        self.files = {}
        for name, stem, reads in files:
            a = self.ann[stem]
            assert all(ci.loadable(a["cov"], rd) for rd in reads), name
            assert stem != "pqr" or all(rd[q + 1] - rd[q] < 1024 for rd in reads for q in range(0, len(rd), 2)), name
            mrf = os.path.join(self.d, name + ".mrf")
            with open(mrf, "w") as h:
                h.write(ci.mrf_text(reads))
            argv = ["0", "t", "./", "LH_GENE_TXT", a["interval"], "UCSC_GENE2ISOFORM", a["map"], "0", "100000000", "MRF_SINGLE", "SHORT_READ", "100", mrf]
            rc, _, exact = ob.run("count", argv)
            assert rc == 0
            oracle = np.array([x for g in exact for x in [g["supports"][0], g["bases"][0]] + g["iso_count"]], np.int64)
            self.files[name] = dict(ann=a, reads=reads, mrf=mrf, oracle=oracle)
        self.rel, self.dev = {}, {}
        self.failed = None

    def release(self, kernel):
        """the release library here: per file the tables, the pools' format and what lsq_debug_check_pool_layout finds"""
        if kernel not in self.rel:
            L.lib.lsq_debug_check_pool_layout.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_ulonglong)]
            L.lib.lsq_debug_check_pool_layout.restype = C.c_int
            out = {}
            for name, f in self.files.items():
                ctx = L.Context(0)
                for k, v in OPTIONS[kernel].items():
                    ctx.set_option(k, v)
                ctx.upload_events(f["ann"]["ev"])
                ctx.upload_reads(0, L.Reads.from_mrf(f["mrf"], f["ann"]["ev"]))
                ctx.count()
                cnt, bases = ctx.counts()
                lay = (C.c_ulonglong * 6)()
                assert L.lib.lsq_debug_check_pool_layout(ctx.h, 0, lay) == 0, (kernel, name, L.lib.lsq_last_error())
                out[name] = dict(cnt=cnt[0].copy(), bases=bases[0].copy(), fmt=ctx.pool_format(0), layout=[int(x) for x in lay],
                                 recounted=ctx.count_status()[1][0], per_look=ctx.launch_info()[0])
                ctx.close()
            self.rel[kernel] = out
        return self.rel[kernel]

    def child(self, kernel):
        """the developer library in a child process: every file on grids of one and of three workgroups"""
        if kernel in self.dev:
            return self.dev[kernel]
        if self.failed:
            # (a child that ended abnormally may have faulted the device: nothing more is started on it from here)
            pytest.fail("the child of %s ended abnormally in an earlier test; no further child is started" % self.failed)
        man = {"options": OPTIONS[kernel], "files": [
            {"name": name, "interval": f["ann"]["interval"], "map": f["ann"]["map"], "mrf": f["mrf"], "R": 100, "grids": [1, 3], "modes": [COUNTERS_ON]}
            for name, f in self.files.items()]}
        mp, op = os.path.join(self.d, kernel + "_manifest.json"), os.path.join(self.d, kernel + "_out.json")
        with open(mp, "w") as h:
            json.dump(man, h)
        env = dict(os.environ, LSQ_LIB=DEV_LIB, LSQ_NO_TORCH="1")
        env.pop("LSQ_OPTIONS", None)
        try:
            p = subprocess.run([sys.executable, CHILD, mp, op], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired as e:
            self.failed = kernel
            pytest.fail("the child of %s ran past %d s: %s" % (kernel, CHILD_TIMEOUT, (e.stderr or b"")[-2000:]))
        if p.returncode != 0:
            self.failed = kernel
            pytest.fail("the child of %s ended with status %d: %s" % (kernel, p.returncode, p.stderr[-2000:]))
        with open(op) as h:
            self.dev[kernel] = json.load(h)
        return self.dev[kernel]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    if not os.path.exists(DEV_LIB):
        pytest.fail("%s is missing: `make -C lesseq_amd/csrc` builds it beside the library" % DEV_LIB)
    return World(tmp_path_factory.mktemp("endrec"))


def check_file(world, kernel, name):
    """the file's tables under `kernel` -- release library, developer library on both grids -- against the oracle's rows and,
    class by class, against the wide records' tables; returns the release library's record of it"""
    f = world.files[name]
    ev = f["ann"]["ev"]
    r = world.release(kernel)[name]
    assert r["recounted"] == 0 and r["fmt"][0] is (kernel != "wide"), (kernel, name, r["fmt"])
    if kernel != "wide":
        assert r["per_look"] == (8 if kernel == "compact8" else 4), (kernel, name)
    assert np.array_equal(table(ev, r["cnt"], r["bases"]), f["oracle"]), (kernel, name, "release library")
    wide = world.release("wide")[name]
    assert np.array_equal(r["cnt"], wide["cnt"]) and np.array_equal(r["bases"], wide["bases"]), (kernel, name, "compact against wide")
    dev = world.child(kernel)[name]
    for grid in (1, 3):
        x = dev["%d/%d" % (grid, COUNTERS_ON)]
        assert x["compact"] == (kernel != "wide") and x["recounted"] == 0, (kernel, name, grid)
        assert np.array_equal(np.asarray(x["cnt"], np.uint64), r["cnt"]) and np.array_equal(np.asarray(x["bases"], np.uint64), r["bases"]), (kernel, name, grid)
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_reads_on_and_beside_every_threshold_at_every_length(world, kernel):
    """ends e - 1, e, e + 1 of both thresholds of one- and two-owner cells, lengths 1, 2, 100 and 1 023"""
    reads = world.files["thresholds"]["reads"]
    one = [rd for rd in reads if len(rd) == 2]
    for t in PQR_ENDS:
        for n in (1, 2, 100, 1023):
            assert {t - 1, t} <= {rd[1] for rd in one if rd[1] - rd[0] == n}, (t, n)
    assert {11101, 11201, 11301} <= {rd[1] for rd in one}
    r = check_file(world, kernel, "thresholds")
    assert r["fmt"][2] == (len(one), len(reads) - len(one), 0)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_every_number_of_padding_records(world, kernel):
    """cells of 1 to 17 reads and junction groups of 1 to 9: each padding count of a last group (0 to 7, 0 to 3), reads that end
    on the thresholds among them, a cell of three whole groups for three workgroups to cut; the layout check finds no group
    over two cells and as many records that are no padding as reads were loaded"""
    pads1, pads2 = set(), set()
    for name in ["pad%02d" % k for k in range(1, 18)] + ["cut"]:
        r = check_file(world, kernel, name)
        reads = world.files[name]["reads"]
        n1 = sum(1 for rd in reads if len(rd) == 2)
        n2 = len(reads) - n1
        assert r["fmt"][2] == (n1, n2, 0), (kernel, name)
        tot1, pad1, mixed1, tot2, pad2, mixed2 = r["layout"]
        assert mixed1 == 0 and mixed2 == 0, (kernel, name, r["layout"])
        assert tot1 - pad1 == n1 and tot2 - pad2 == n2, (kernel, name, r["layout"])
        assert tot1 % 8 == 0 and tot2 % 4 == 0, (kernel, name, r["layout"])
        if name != "cut":
            k = int(name[3:])
            j = (k - 1) % 9 + 1
            # (the file's groups: the two cells' reads and the two junctions' -- what their last groups are padded by)
            assert pad1 == (-k) % 8 + (-(18 - k)) % 8, (kernel, name, r["layout"])
            assert pad2 == (-j) % 4 + (-(10 - j)) % 4 + (-plain_group(k)) % 4, (kernel, name, r["layout"])
            pads1 |= {(-k) % 8, (-(18 - k)) % 8}
            pads2 |= {(-j) % 4, (-(10 - j)) % 4}
        else:
            assert (tot1, pad1) == (24, 0)
    assert pads1 == set(range(8)) and pads2 == set(range(4))


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_block_ends_on_both_sides_of_22_bits(world, kernel):
    """a bucket of more than 2 Mi bases: block ends and second-block reaches of 2^22 - 2 .. 2^22 + 1 are kept as compact
    records or handed to the third pool as compact_block_fits says on the host, the file stays compact, and the tables
    are the oracle's"""
    f = world.files["edge22"]
    want = expected_pools(f["reads"], G_LO)
    # the edge itself: of the four ends only 2^22 - 2 fits (2^22 - 1 is the padding's), as an end and as a reach
    assert [fits((1 << 22) + d - 50, 50) for d in (-2, -1, 0, 1)] == [True, False, False, False]
    assert 0 < want[2] * 16 <= sum(want) and want[2] == 3 * (3 + 1 + 1)
    r = check_file(world, kernel, "edge22")
    if kernel == "wide":
        assert r["fmt"][0] is False and r["fmt"][2] == (want[0] + 9, want[1] + 6, 0)
    else:
        assert r["fmt"][0] is True and r["fmt"][2] == want, (kernel, r["fmt"], want)
    assert r["layout"][2] == 0 and r["layout"][5] == 0
    assert r["layout"][0] - r["layout"][1] == r["fmt"][2][0] and r["layout"][3] - r["layout"][4] == r["fmt"][2][1]


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS[1:])
def test_replay_reads_the_new_records_back(kernel, tmp_path):
    """two read files, every event with an EM loop replayed over its valid reads in index order (guard band 1.0): theta,
    log-likelihood and iteration counts equal the oracle's bit for bit"""
    import test_parity_gpu as tp
    spec = L.SynthSpec(seed=31, n_events=30, n_reads=4000, read_length=100, n_chrom=1)
    L.synth_write(spec, str(tmp_path), "s", write_mrf=True)
    with open(tmp_path / "s.mrf") as h:
        lines = h.read().split("\n")
    head, body = lines[0], [ln for ln in lines[1:] if ln]
    with open(tmp_path / "s2.mrf", "w") as h:
        h.write("\n".join([head] + body[::3]) + "\n")
    argv = ["0", "s", "./", "LH_GENE_TXT", str(tmp_path / "s.interval"), "UCSC_GENE2ISOFORM", str(tmp_path / "s.map"), "0", "100000000",
            "MRF_SINGLE", "SHORT_READ", "100", str(tmp_path / "s.mrf"), str(len(body) * 100),
            "MRF_SINGLE", "SHORT_READ", "100", str(tmp_path / "s2.mrf"), str(len(body[::3]) * 100)]
    rc, _, exact = ob.run("solve", argv)
    assert rc == 0
    n = tp.compare_exact(tp.gpu_exact(argv, band=1.0, options=OPTIONS[kernel]), exact, kernel)
    assert n > 10
