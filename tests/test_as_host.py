"""test_as without a device: the matrix and table readers, the input errors of the executable (exit 1, reported before
any HIP call) and R's number formatting (include/lesseq_hip.h: lsq_as_read_*, lsq_as_format_number)."""
import math
import os

import numpy as np
import pytest

import lesseq_amd as L
from lesseq_amd import diffsplice as ds

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_matrix_reader_skips_header_and_reads_na_and_inf(tmp_path):
    p = _write(tmp_path, "v.txt", "ID\tc1a\tc1b\tc2a\tc2b\n"
               "f1\t1\tNA\tNaN\tnan\n"
               "f2\t-nan\tInf\t-Inf\tinf\n"
               "f3\t-inf\t2.5\t1e3\t-0.25\n")
    inp = ds.read_matrix("wilcox", [p], 2, 2)
    assert inp.ids == ["f1", "f2", "f3"]
    v = inp.values
    assert v.shape == (3, 4)
    assert v[0, 0] == 1.0 and np.isnan(v[0, 1:]).all()
    assert np.isnan(v[1, 0]) and v[1, 1] == math.inf and v[1, 2] == -math.inf and v[1, 3] == math.inf
    assert v[2, 0] == -math.inf and list(v[2, 1:]) == [2.5, 1000.0, -0.25]
    assert inp.totals is None


def test_fisher_matrix_pairs_rows_and_ignores_an_odd_last_row(tmp_path):
    p = _write(tmp_path, "c.txt", "ID\ts1\ts2\nA.inc\t5\t6\nA.skp\t7\t8\nB.inc\t1\tNA\nB.skp\t2\t3\nC.inc\t9\t9\n")
    inp = ds.read_matrix("fisher", [p])
    assert inp.ids == ["A.skp", "B.skp"]
    assert inp.values[0].tolist() == [5, 6, 7, 8]
    assert inp.values[1, 0] == 1 and np.isnan(inp.values[1, 1]) and inp.values[1, 2:].tolist() == [2, 3]


def _cli_input_error(argv, capfd, *needles):
    rc, text = L.cli_run("test_as", argv)
    err = capfd.readouterr().err
    # exit 1 with the message on a machine with a GPU and on one without: no device was opened for it
    assert rc == 1, (rc, err)
    assert text == ""
    for n in needles:
        assert n in err, (n, err)


def test_input_errors_exit_1(tmp_path, capfd):
    good = _write(tmp_path, "good.txt", "ID\ta\tb\tc\td\nf1\t1\t2\t3\t4\nf2\t5\t6\t7\t8\n")
    out = str(tmp_path / "out.txt")
    ragged = _write(tmp_path, "ragged.txt", "ID\ta\tb\tc\td\nf1\t1\t2\t3\t4\nf2\t5\t6\t7\n")
    _cli_input_error(["wilcox", ragged, "2", "2", out], capfd, "ragged.txt:3")
    dup = _write(tmp_path, "dup.txt", "ID\ta\tb\tc\td\nf1\t1\t2\t3\t4\nf1\t5\t6\t7\t8\n")
    _cli_input_error(["wilcox", dup, "2", "2", out], capfd, "dup.txt:3", "duplicate")
    word = _write(tmp_path, "word.txt", "ID\ta\tb\tc\td\nf1\t1\t2\tthree\t4\n")
    _cli_input_error(["wilcox", word, "2", "2", out], capfd, "word.txt:2", "three")
    empty = _write(tmp_path, "empty.txt", "ID\ta\tb\tc\td\nf1\t1\t\t3\t4\n")
    _cli_input_error(["wilcox", empty, "2", "2", out], capfd, "empty.txt:2")
    other = _write(tmp_path, "other.txt", "ID\ta\tb\tc\td\nf1\t1\t2\t3\t4\nf3\t5\t6\t7\t8\n")
    _cli_input_error(["lrt", good, other, "2", "2", out], capfd, "other.txt:3", "f3")
    _cli_input_error(["wilcox", good, "1", "2", out], capfd, "good.txt:2")             # n1 + n2 != columns
    _cli_input_error(["lrt", good, good, "3", "2", out], capfd, "good.txt:2")
    neg = _write(tmp_path, "neg.txt", "ID\ta\tb\tc\td\nf1\t1\t2\t-3\t4\nf2\t5\t6\t7\t8\n")
    _cli_input_error(["lrt", good, neg, "2", "2", out], capfd, "neg.txt:2", "negative")
    _cli_input_error(["lrt", neg, good, "2", "2", out], capfd, "neg.txt:2", "negative")
    fneg = _write(tmp_path, "fneg.txt", "ID\ts1\ts2\nA.inc\t5\t-6\nA.skp\t7\t8\n")
    _cli_input_error(["fisher", fneg, out], capfd, "fneg.txt:2", "negative")
    # a negative value is fine for Wilcoxon (relative expression levels are not counts)
    assert ds.read_matrix("wilcox", [neg], 2, 2).values[0, 2] == -3
    _cli_input_error(["wilcox", str(tmp_path / "missing.txt"), "2", "2", out], capfd, "missing.txt")
    _cli_input_error(["wilcox", good, "0", "4", out], capfd, "n1 and n2")
    _cli_input_error(["median", good, out], capfd, "Usage")
    _cli_input_error(["lrt", "--tables", "2", "2", out, os.path.join(GOLD, "toy", "count.out")], capfd, "4 tables expected")
    assert not os.path.exists(out)


def test_tables_whose_ids_differ_exit_1(tmp_path, capfd):
    a = os.path.join(GOLD, "toy", "count.out")
    lines = open(a).read().splitlines(True)
    b = _write(tmp_path, "b.out", "".join(lines[:3]) + lines[3].replace("SE1.skp", "SE1.alt"))
    _cli_input_error(["fisher", "--tables", "-", a, b], capfd, "b.out:4", "SE1.alt")
    c = _write(tmp_path, "c.out", "".join(lines[:3]))
    _cli_input_error(["fisher", "--tables", "-", a, c], capfd, "different form IDs")
    with pytest.raises(L.LsqError):
        ds.read_tables("lrt", [a, b], 1, 1)


def test_fisher_tables_from_toy_count():
    a = os.path.join(GOLD, "toy", "count.out")
    inp = ds.read_tables("fisher", [a, a])
    assert inp.ids == ["RI1.spl", "SE1.skp"]
    assert inp.values.tolist() == [[3, 3, 3, 3], [5, 5, 3, 3]]
    assert inp.left_out == 0


def _rows(path):
    return [line.rstrip("\n").split("\t") for line in open(path)]


def test_three_form_event_left_out_of_fisher_kept_for_lrt():
    a = os.path.join(GOLD, "wild_s13", "count.out")
    rows = _rows(a)
    genes = [r[0] for r in rows]
    sizes = {g: genes.count(g) for g in genes}
    assert sizes["10"] == 3
    f = ds.read_tables("fisher", [a, a])
    two = [g for g in dict.fromkeys(genes) if sizes[g] == 2]
    assert f.left_out == len(sizes) - len(two) and f.left_out >= 1
    assert len(f.ids) == len(two)
    assert not any(i.startswith("10_") for i in f.ids)
    lrt = ds.read_tables("lrt", [a, a, a, a], 2, 2)
    assert lrt.ids == [r[2] for r in rows]
    assert {"10_i0", "10_i1", "10_i2"} <= set(lrt.ids)
    for i, r in enumerate(rows):
        assert lrt.values[i].tolist() == [float(r[3])] * 4
        assert lrt.totals[i].tolist() == [float(r[1])] * 4


def test_multi_method_totals_are_summed():
    a = os.path.join(GOLD, "multi_method", "count.out")
    rows = _rows(a)
    assert all(len(r) == 5 for r in rows)           # M = 2: gene, two totals, form, count
    inp = ds.read_tables("lrt", [a, a], 1, 1)
    for i, r in enumerate(rows):
        assert inp.ids[i] == r[3]
        assert inp.totals[i].tolist() == [float(r[1]) + float(r[2])] * 2
        assert inp.values[i].tolist() == [float(r[4])] * 2
    s = os.path.join(GOLD, "multi_method", "solve.out")
    srows = _rows(s)
    w = ds.read_tables("wilcox", [s, s], 1, 1)
    assert w.values[:, 0].tolist() == [float(r[4]) for r in srows]


def test_formatter_examples():
    cases = {1e-4: "1e-04", 0.001: "0.001", 1e5: "1e+05", 123456.0: "123456", 1 / 3: "0.333333333333333",
             0.0: "0", 1.0: "1", float("nan"): "NA", 0.5: "0.5", 2.5e-300: "2.5e-300", 1e-15: "1e-15",
             0.1 + 0.2: "0.3", -1e-5: "-1e-05", 1e15: "1e+15", 123456.7: "123456.7", 0.0001234: "0.0001234"}
    for v, s in cases.items():
        assert ds.format_number(v) == s, (v, ds.format_number(v), s)
