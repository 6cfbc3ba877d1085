"""events / classify without a device: classify for genes past 64 segments, Events.r's gene-list conversion and order,
the .matrix reader, R's counter text, and the input errors of the events executable (exit 1, nothing printed, no file
touched, reported before any HIP call)."""
import json
import os
import subprocess

import pytest

import lesseq_amd as L
from lesseq_amd import diffsplice as ds
from lesseq_amd import localevents as le

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
BIN = os.path.join(os.path.dirname(HERE), "lesseq_amd", "bin")


def _matrix(d, name, header, rows):
    with open(os.path.join(d, name + ".matrix"), "w") as f:
        f.write(header + "\n" + "".join("".join("%d\t" % v for v in r) + "\n" for r in rows))


SE3 = "chr1\t+\t[1000,1100)-[1200,1300)-[1500,1600)-"


def test_classify_wide_matches_reference(tmp_path):
    """genes with more than 64 atomic segments (WIDE: 96) are written, byte for byte what the reference's classify wrote"""
    d = os.path.join(GOLD, "wide")
    c = json.load(open(os.path.join(d, "classify.json")))["classify"]
    out = tmp_path / "classify"
    out.mkdir()
    argv = list(c["argv"])
    argv[2] = str(out) + "/"
    argv[4], argv[6] = os.path.join(d, argv[4]), os.path.join(d, argv[6])
    rc, _ = L.cli_run("classify", argv)
    assert rc == c["exit"] == 0
    assert sorted(os.listdir(out)) == c["files"]
    for fn in c["files"]:
        assert open(out / fn).read() == open(os.path.join(d, "classify", fn)).read(), fn
    head = open(out / "WIDE.matrix").readline()
    assert head.count("[") > 64


def test_numeric_ids_sort_numerically():
    """events_s1's ids are 1..40: R reads them as integers, table() sorts 1, 2, ..., 40"""
    d = os.path.join(GOLD, "events_s1")
    g = le.Graphs.from_matrices(os.path.join(d, "classify") + "/", os.path.join(d, "ev.map"))
    assert g.names() == [str(i) for i in range(1, 41)]


def test_id_conversion(tmp_path):
    d = str(tmp_path)
    for n in ("1", "2", "10", "1.5", "B", "a", "b", "a1"):
        _matrix(d, n, SE3, [[1, 1, 1], [1, 0, 1]])
    grp = tmp_path / "g.map"
    # integers: "01" and "1" are one gene, "10" after "2"; an unterminated last line is read
    grp.write_text("10\tx\n01\ty\n2\tz\n2\tw\n1\tv\n10\tu")
    assert le.Graphs.from_matrices(d + "/", str(grp)).names() == ["1", "2", "10"]
    # decimal numbers: doubles, printed as.character
    grp.write_text("1.50\tx\n1.5\ty\n2\tz\n2.0\tw\n")
    assert le.Graphs.from_matrices(d + "/", str(grp)).names() == ["1.5", "2"]
    # strings: byte order (LC_COLLATE=C); a single-line id is left out
    grp.write_text("b\t1\nb\t2\na\t1\na\t2\nB\t1\nB\t2\na1\t1\n")
    assert le.Graphs.from_matrices(d + "/", str(grp)).names() == ["B", "a", "b"]


def test_header_positions_and_shapes(tmp_path):
    d = str(tmp_path)
    _matrix(d, "neg", "chr1\t-\t[-5,10)-[20,30)-[40,50)-", [[1, 1, 1], [1, 0, 1]])
    _matrix(d, "two", "chr1\t+\t[1,2)-[3,4)-", [[1, 1], [1, 0]])
    _matrix(d, "one", SE3, [[1, 0, 1]])
    (tmp_path / "g").write_text("neg\ta\nneg\tb\ntwo\ta\ntwo\tb\none\ta\none\tb\n")
    g = le.Graphs.from_matrices(d + "/", str(tmp_path / "g"))
    assert g.names() == ["neg", "one", "two"]
    assert g.positions(0) == [5, 10, 20, 30, 40, 50]          # the minus sign is not part of a digit run
    assert g.shape(1) == (3, 1)                               # a single isoform row
    assert g.shape(2) == (2, 2) and g.positions(2) == []      # ncol < 3: kept (printed), skipped


@pytest.mark.parametrize("v,text", [(99999, "99999"), (100000, "1e+05"), (100001, "100001")])
def test_counter_text(v, text):
    assert ds.format_number(float(v)) == text


def _events_proc(argv, cwd):
    return subprocess.run([os.path.join(BIN, "events")] + argv, cwd=cwd, capture_output=True, text=True)


def _assert_refused(p, out_dir, *needles):
    assert p.returncode == 1, (p.returncode, p.stderr)
    assert p.stdout == ""
    assert os.listdir(out_dir) == []
    for n in needles:
        assert n in p.stderr, (n, p.stderr)


def test_input_errors_exit_1(tmp_path):
    out = tmp_path / "out"
    out.mkdir()
    # classify_mix: `cut` has two map lines (the second unterminated) but classify wrote no cut.matrix
    d = os.path.join(GOLD, "classify_mix")
    p = _events_proc([os.path.join(d, "classify") + "/", os.path.join(d, "cm.map"), str(out) + "/ev_"], d)
    _assert_refused(p, out, "cut.matrix")
    # "007" is the integer 7 to R: it reads 7.matrix, and only 007.matrix exists
    m = tmp_path / "m"
    m.mkdir()
    _matrix(str(m), "007", SE3, [[1, 1, 1], [1, 0, 1]])
    (tmp_path / "g7").write_text("007\ta\n007\tb\n")
    p = _events_proc([str(m) + "/", str(tmp_path / "g7"), str(out) + "/ev_"], str(tmp_path))
    _assert_refused(p, out, "7.matrix")
    # no gene with more than one line
    (tmp_path / "g1").write_text("007\ta\n")
    p = _events_proc([str(m) + "/", str(tmp_path / "g1"), str(out) + "/ev_"], str(tmp_path))
    _assert_refused(p, out, "g1")
    # a malformed row names file and line
    _matrix(str(m), "bad", SE3, [[1, 1, 1], [1, 2, 1]])
    (tmp_path / "gb").write_text("bad\ta\nbad\tb\n")
    p = _events_proc([str(m) + "/", str(tmp_path / "gb"), str(out) + "/ev_"], str(tmp_path))
    _assert_refused(p, out, "bad.matrix:3")
    # an output directory that does not exist
    (tmp_path / "g2").write_text("007\ta\n007\tb\n")
    _matrix(str(m), "7", SE3, [[1, 1, 1], [1, 0, 1]])
    p = _events_proc([str(m) + "/", str(tmp_path / "g2"), str(tmp_path / "nowhere" / "ev_")], str(tmp_path))
    _assert_refused(p, out, "nowhere")
