"""SAM_SINGLE on the host (CPU only): the converter to the equivalent MRF (lsq_sam_to_mrf, the sam2mrf executable) and the
host parser (lsq_sam_parse) against the fixtures of tests/golden/sam -- SAM inputs, their MRF equivalents made by the
independent pure-Python converter of tools/make_sam_golden.py, and the reference's output on those.  Every case
directory is run; none is skipped."""
import json
import os
import subprocess

import numpy as np
import pytest

import lesseq_amd as L

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "sam")
BIN = os.path.join(os.path.dirname(HERE), "lesseq_amd", "bin")
SAM_CASES = sorted(d for d in os.listdir(GOLD) if os.path.isdir(os.path.join(GOLD, d))) if os.path.isdir(GOLD) else []
LSQ_E_PARSE = -4


def load(name):
    d = os.path.join(GOLD, name)
    return json.load(open(os.path.join(d, "case.json"))), d


def read(path):
    with open(path, "rb") as f:
        return f.read()


def strand_strings(ev, ids):
    names = {int(i): L.lib.lsq_events_strand_name(ev.h, int(i)) for i in np.unique(ids)}
    assert None not in names.values()
    return [names[int(i)] for i in ids]


def same_reads(ev, a, b):
    """two read sets parsed against the same events: every array equal, strands compared as strings"""
    x, y = a.arrays(), b.arrays()
    assert len(a) == len(b) and a.num_blocks == b.num_blocks
    for k, what in enumerate(("blk_off", "line_no", "blk_start", "blk_end", "blk_chrom")):
        assert np.array_equal(x[k], y[k]), what
    assert strand_strings(ev, x[5]) == strand_strings(ev, y[5])


def events_of(d, R=100, rtype="SHORT_READ"):
    return L.Events(L.Annotation(os.path.join(d, "x.interval"), os.path.join(d, "x.map"), 0, 10 ** 9), (rtype,), (R,))


def test_the_golden_set_is_complete():
    assert SAM_CASES == ["basic", "cigar", "filters", "multi", "names"]
    for name in SAM_CASES:
        c, d = load(name)
        assert c["conversions"] and c["runs"]
        for r in c["runs"]:
            assert os.path.isfile(os.path.join(d, r["stdout"])) and r["exit"] == 0
    assert len(load("filters")[0]["conversions"]) == 3
    big = read(os.path.join(GOLD, "cigar", "in.sam")).split(b"\n")
    assert max(len(ln) for ln in big) > 8192 and any(ln.split(b"\t")[5].count(b"M") >= 150 for ln in big if ln.count(b"\t") >= 5)
    assert not read(os.path.join(GOLD, "basic", "in.sam")).endswith(b"\n")


@pytest.mark.parametrize("name", SAM_CASES)
def test_converter_gives_the_committed_mrf(name, tmp_path):
    """lsq_sam_to_mrf and the sam2mrf executable (from a file and from standard input) on every in.sam give the MRF the
    independent Python converter wrote, byte for byte"""
    c, d = load(name)
    for cv in c["conversions"]:
        sam, want = read(os.path.join(d, cv["sam"])), read(os.path.join(d, cv["mrf"]))
        assert L.sam_to_mrf(sam, cv["skip_flags"], cv["min_mapq"]) == want, cv
        opts = ["--skip-flags", str(cv["skip_flags"]), "--min-mapq", str(cv["min_mapq"])]
        p = subprocess.run([os.path.join(BIN, "sam2mrf")] + opts + [os.path.join(d, cv["sam"])], capture_output=True)
        assert p.returncode == 0 and p.stdout == want, (cv, p.stderr)
        p = subprocess.run([os.path.join(BIN, "sam2mrf")] + opts, input=sam, capture_output=True)
        assert p.returncode == 0 and p.stdout == want, (cv, p.stderr)
    if all(cv["skip_flags"] == L.SAM_DEFAULT_SKIP_FLAGS and cv["min_mapq"] == 0 for cv in c["conversions"]):
        p = subprocess.run([os.path.join(BIN, "sam2mrf"), os.path.join(d, "in.sam")], capture_output=True)
        assert p.returncode == 0 and p.stdout == read(os.path.join(d, "in.mrf"))


@pytest.mark.parametrize("name", SAM_CASES)
def test_host_parser_gives_the_arrays_of_the_equivalent_mrf(name):
    c, d = load(name)
    for cv in c["conversions"]:
        ev = events_of(d)
        a = L.Reads.from_sam(os.path.join(d, cv["sam"]), ev, cv["skip_flags"], cv["min_mapq"])
        b = L.Reads.from_mrf(os.path.join(d, cv["mrf"]), ev)
        assert len(a) > 50
        same_reads(ev, a, b)
        same_reads(ev, a, L.Reads.from_sam(os.path.join(d, cv["sam"]), ev, cv["skip_flags"], cv["min_mapq"], n_threads=1))
    ev = events_of(d)
    same_reads(ev, L.Reads.from_mrf(os.path.join(d, "in.sam"), ev, read_format="SAM_SINGLE"), L.Reads.from_mrf(os.path.join(d, "in.mrf"), ev))


GOOD = "q\t0\tchr1\t1101\t60\t50M\t*\t0\t0\t" + "A" * 50 + "\t" + "I" * 50 + "\tNH:i:1"
# every malformed-line kind of the format: (name, the line)
BAD_LINES = [
    ("five_fields", "q\t0\tchr1\t1101\t60"),
    ("empty_line", ""),
    ("no_tab_at_all", "just some text"),
    ("flag_not_a_number", "q\t0x10\tchr1\t1101\t60\t50M\t*"),
    ("flag_empty", "q\t\tchr1\t1101\t60\t50M\t*"),
    ("flag_signed", "q\t+0\tchr1\t1101\t60\t50M\t*"),
    ("flag_above_65535", "q\t65536\tchr1\t1101\t60\t50M\t*"),
    ("flag_bad_on_an_unmapped_looking_record", "q\t4x\t*\t0\t0\t*\t*"),
    ("mapq_not_a_number", "q\t0\tchr1\t1101\t6o\t50M\t*"),
    ("mapq_above_255", "q\t0\tchr1\t1101\t256\t50M\t*"),
    ("mapq_bad_on_a_skipped_flag", "q\t4\tchr1\t1101\t-1\t50M\t*"),
    ("pos_not_a_number", "q\t0\tchr1\t11o1\t60\t50M\t*"),
    ("pos_negative", "q\t0\tchr1\t-5\t60\t50M\t*"),
    ("pos_above_2_31", "q\t0\tchr1\t2147483648\t60\t50M\t*"),
    ("pos_bad_with_unknown_chromosome", "q\t0\tnowhere\t1.5\t60\t50M\t*"),
    ("pos_bad_with_rname_star", "q\t0\t*\tx\t60\t50M\t*"),
    ("cigar_empty", "q\t0\tchr1\t1101\t60\t\t*"),
    ("cigar_no_length", "q\t0\tchr1\t1101\t60\tM\t*"),
    ("cigar_unknown_operator", "q\t0\tchr1\t1101\t60\t50M3B\t*"),
    ("cigar_lower_case", "q\t0\tchr1\t1101\t60\t50m\t*"),
    ("cigar_trailing_digits", "q\t0\tchr1\t1101\t60\t50M3\t*"),
    ("cigar_star_inside", "q\t0\tchr1\t1101\t60\t50M*\t*"),
    ("cigar_length_above_2_31", "q\t0\tchr1\t1101\t60\t2147483648M\t*"),
    ("cigar_bad_with_pos_zero", "q\t0\tchr1\t0\t60\t5Q\t*"),
    ("cigar_bad_at_line_end", "q\t0\tchr1\t1101\t60\t50M!"),
    ("reference_end_beyond_2_31", "q\t0\tchr1\t2147483647\t60\t2M\t*"),
    ("reference_end_beyond_2_31_by_a_gap", "q\t0\tchr1\t2000000000\t60\t10M2147483647N\t*"),
]
# lines that look odd and are NOT malformed (they make no read, or a read)
FINE_LINES = ["q\t4\t*\t0\t0\t*", "q\t0\t*\t0\t0\t*\t*\t0\t0\t*\t*", "q\t0\tchr1\t0\t60\t50M", "q\t0\tchr1\t1101\t60\t*", "@", "@CO", "q\t00016\tchr1\t0001101\t060\t050M",
              "q\t2048\tchr1\t1101\t0\t50M", "\t0\tchr1\t1101\t60\t50M", "q\t0\t\t1101\t60\t50M", "q\t0\tchr1\t2147483647\t60\t1M", "q\t0\tchr1\t2147483647\t60\t1S1I1H",
              "q\t0\tchr1:1\t1101\t60\t50M", "q\t0\tchr1\t1101\t60\t50M\t"]


def bad_file(line, second):
    """several hundred good lines, the bad one late, a second bad one behind it"""
    lines = ["@HD\tVN:1.6", "@SQ\tSN:chr1\tLN:100000"] + [GOOD] * 400 + FINE_LINES + [GOOD] * 37 + [line] + [GOOD] * 20 + [second] + [GOOD] * 5
    return "\n".join(lines) + "\n", 2 + 400 + len(FINE_LINES) + 37 + 1


@pytest.mark.parametrize("kind,line", BAD_LINES, ids=[k for k, _ in BAD_LINES])
def test_malformed_lines_report_the_first_bad_line(kind, line, tmp_path):
    second = BAD_LINES[0][1] if kind != "five_fields" else BAD_LINES[3][1]
    text, k = bad_file(line, second)
    path = tmp_path / "bad.sam"
    path.write_text(text)
    d = os.path.join(GOLD, "cigar")
    ev = events_of(d, 50)
    want = "#%d:%s" % (k, line)
    for n_threads in (1, 0):
        with pytest.raises(L.LsqError) as e:
            L.Reads.from_sam(str(path), ev, n_threads=n_threads)
        assert e.value.status == LSQ_E_PARSE and str(e.value).endswith(": " + want), (kind, str(e.value))
    with pytest.raises(L.LsqError) as e:
        L.sam_to_mrf(text.encode())
    assert e.value.status == LSQ_E_PARSE and str(e.value).endswith(": " + want)
    p = subprocess.run([os.path.join(BIN, "sam2mrf"), str(path)], capture_output=True, text=True)
    assert p.returncode == 1 and p.stdout == "" and want in p.stderr and "Lexical_cast error" in p.stderr
    # the same file without its bad lines parses, and the odd-looking lines in it are what the Python converter says
    good = "\n".join(ln for ln in text.split("\n")[:-1] if ln not in (line, second)) + "\n"
    (tmp_path / "good.sam").write_text(good)
    assert len(L.Reads.from_sam(str(tmp_path / "good.sam"), ev)) > 400


def test_odd_lines_that_are_not_malformed():
    got = L.sam_to_mrf(("\n".join(FINE_LINES) + "\n").encode()).decode().split("\n")
    assert got[0] == "AlignmentBlocks" and got[-1] == ""
    assert got[1:-1] == ["#", "#", "#", "#", "#", "#", "chr1:-:1101:1150:1:50", "#", "chr1:+:1101:1150:1:50", ":+:1101:1150:1:50", "chr1:+:2147483647:2147483647:1:1", "#",
                         "#", "chr1:+:1101:1150:1:50"]
    # a last line without a newline is never seen; an empty text is a header alone
    assert L.sam_to_mrf(b"@HD\n" + GOOD.encode()) == b"AlignmentBlocks\n#\n"
    assert L.sam_to_mrf(b"") == b"AlignmentBlocks\n"
    assert L.sam_to_mrf(("q\t16\tc\t11\t0\t5S10M2I3D10=100N2X1P8M5H\n").encode()) == b"AlignmentBlocks\nc:-:11:33:6:27,c:-:134:143:28:37\n"


def test_new_entry_points_are_exported_and_the_abi_version_stays():
    for sym in ("lsq_sam_parse", "lsq_sam_to_mrf", "lsq_last_ingest_stage_name", "lsq_last_sam_paths", "lsq_synth_write_sam"):
        assert hasattr(L.lib, sym), sym
    assert L.lib.lsq_abi_version() == 2
    header = open(os.path.join(os.path.dirname(HERE), "include", "lesseq_hip.h")).read()
    for sym in ("lsq_sam_parse", "lsq_sam_to_mrf", "lsq_last_ingest_stage_name", "lsq_last_sam_paths", "lsq_synth_write_sam"):
        assert sym + "(" in header
    assert "#define LSQ_ABI_VERSION 2" in header


def test_unknown_formats_still_give_the_old_message(tmp_path):
    d = os.path.join(GOLD, "basic")
    ev = events_of(d)
    for fmt in ("SAM", "SAM_PAIRED", "sam_single", "BAM_SINGLE", "MRF_PAIRED"):
        with pytest.raises(L.LsqError) as e:
            L.Reads.from_mrf(os.path.join(d, "in.sam"), ev, read_format=fmt)
        assert e.value.status == -3 and str(e.value).endswith("Unknown file format error: " + fmt)
    with pytest.raises(L.LsqError) as e:
        L.Reads.from_sam(str(tmp_path / "missing.sam"), ev)
    assert e.value.status == -2


def test_synthetic_sam_is_the_synthetic_mrf(tmp_path):
    """lsq_synth_write_sam writes the reads of lsq_synth_write: behind its header lines, the converter gives the MRF file line by
    line (but for the generator's few reads whose second block lies ahead of its first, which a CIGAR cannot say)"""
    spec = L.SynthSpec(11, 300, 20000, 100, 3, L.EVENT_TYPES, zipf=True)
    L.synth_write(spec, str(tmp_path), "m")
    L.synth_write_sam(spec, str(tmp_path), "s")
    assert read(str(tmp_path / "m.interval")) == read(str(tmp_path / "s.interval")) and read(str(tmp_path / "m.map")) == read(str(tmp_path / "s.map"))
    sam = read(str(tmp_path / "s.sam"))
    n_head = sum(1 for ln in sam.split(b"\n") if ln.startswith(b"@"))
    assert n_head == 2 + 3
    got = L.sam_to_mrf(sam).split(b"\n")
    want = read(str(tmp_path / "m.mrf")).split(b"\n")
    assert got[1:1 + n_head] == [b"#"] * n_head and len(got) == len(want) + n_head
    differ = [k for k in range(1, len(want) - 1) if got[k + n_head] != want[k]]
    assert len(differ) < 0.01 * len(want)
    for k in differ:
        assert want[k].startswith(got[k + n_head] + b",")
    rec = sam.split(b"\n")[n_head].split(b"\t")
    assert len(rec) >= 13 and len(rec[9]) == 100 and len(rec[10]) == 100
