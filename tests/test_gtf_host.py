"""Annotation from GTF, the part that needs no GPU: the restatement in gtf_ref.py is pinned to the reference (it must
reproduce every fixture of tests/golden/gtf/, which hold what the reference's own parseGencode and gencodeIsoformMap
printed), and gencodeIsoformMap -- through the library, through cli_run and as a process -- against the same fixtures."""
import ctypes as C
import os
import re
import subprocess

import pytest

import lesseq_amd as L
from lesseq_amd import gencode
import gtf_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "gtf")
BIN = os.path.join(ROOT, "lesseq_amd", "bin")

GTF_CASES = sorted(os.path.relpath(d, GOLD) for d, _, fs in os.walk(GOLD) if "in.gtf" in fs)
PARSED = [c for c in GTF_CASES if os.path.exists(os.path.join(GOLD, c, "out.map"))]
MAPNAMES = sorted(f[:-len(".names")] for f in os.listdir(os.path.join(GOLD, "mapnames")) if f.endswith(".names"))


def rd(*parts):
    with open(os.path.join(GOLD, *parts), "rb") as f:
        return f.read()


def name_lists():
    return [(c, rd(c, "names.txt"), rd(c, "out.map")) for c in PARSED] + \
           [("mapnames/" + m, rd("mapnames", m + ".names"), rd("mapnames", m + ".map")) for m in MAPNAMES]


def test_fixture_sets_are_complete():
    assert {"cuff", "gencode", "numbers"} <= set(GTF_CASES)
    errs = [c for c in GTF_CASES if c.startswith("errors/")]
    messages = {rd(c, "out.stderr") for c in errs}
    assert len(errs) >= 4 and len(messages) >= 4 and all(m.startswith(b"PROBLEM: ") for m in messages)
    assert all(rd(c, "status") == b"1\n" and rd(c, "out.interval") == b"" for c in errs)
    assert all(rd(c, "status") == b"0\n" for c in PARSED) and len(PARSED) == 3
    assert {"returning_gene", "several_bars", "tab_in_line", "no_final_newline"} <= set(MAPNAMES)
    assert not rd("gencode", "in.gtf").endswith(b"\n") and b"\n#" not in rd("gencode", "in.gtf")
    assert max(len(l) for l in rd("gencode", "in.gtf").split(b"\n")) > 10000


@pytest.mark.parametrize("case", GTF_CASES)
def test_restatement_reproduces_the_reference(case):
    rc, out, err = R.parse_gencode(rd(case, "in.gtf"))
    assert rc == int(rd(case, "status"))
    assert err == rd(case, "out.stderr")
    assert out == rd(case, "out.interval")
    if rc == 0:
        assert R.cut_f1(out) == rd(case, "names.txt")


@pytest.mark.parametrize("case,names,want", name_lists(), ids=[c for c, _, _ in name_lists()])
def test_isoform_map_equals_the_reference(case, names, want, tmp_path):
    assert R.isoform_map(names) == (0, want, b"")
    assert gencode.isoform_map(names) == want
    path = tmp_path / "names.txt"
    path.write_bytes(names)
    rc, text = L.cli_run("gencodeIsoformMap", [str(path)])
    assert rc == 0 and text.encode() == want
    p = subprocess.run([os.path.join(BIN, "gencodeIsoformMap")], input=names, capture_output=True, timeout=60)
    assert (p.returncode, p.stdout, p.stderr) == (0, want, b"")
    p = subprocess.run([os.path.join(BIN, "gencodeIsoformMap"), str(path)], capture_output=True, timeout=60)
    assert (p.returncode, p.stdout, p.stderr) == (0, want, b"")


def test_two_key_order_and_counter_rules():
    names = b"B|x\nG|x\nG-1|x\nG.1|x\nG10|x\nG2|X\nG2|x\na|x\n"
    assert gencode.isoform_map(names) == b"".join(b"%d\t%s\n" % (n, l) for n, l in zip([1, 2, 3, 4, 5, 6, 6, 7], names.split(b"\n")))
    assert gencode.isoform_map(b"G1|a\nG1|b\nG2|c\nG1|d") == b"1\tG1|a\n1\tG1|b\n2\tG2|c\n3\tG1|d\n"
    assert gencode.isoform_map(b"") == b"" and gencode.isoform_map(b"\n\n") == b""


@pytest.mark.parametrize("names,line", [(b"G|a\nnobar\nG|b\n", 2), (b"nobar\nG|a\n", 1), (b"G|a\n\n\r\n \nG|b\n", 4), (b"G|a\nH|b\nlast", 3)])
def test_map_input_without_bar_is_an_input_error(names, line, tmp_path):
    want_err = b"PROBLEM: line %d has no '|' between gene and transcript id\n" % line
    assert R.isoform_map(names) == (1, b"", want_err)
    p = subprocess.run([os.path.join(BIN, "gencodeIsoformMap")], input=names, capture_output=True, timeout=60)
    assert (p.returncode, p.stdout, p.stderr) == (1, b"", want_err)
    path = tmp_path / "n"
    path.write_bytes(names)
    rc, text = L.cli_run("gencodeIsoformMap", [str(path)])
    assert rc == 1 and text == ""
    with pytest.raises(L.LsqError) as e:
        gencode.isoform_map(names)
    assert e.value.status == -4 and ("line %d " % line) in str(e.value)


def test_new_declarations_are_exported_and_abi_stays():
    header = open(os.path.join(ROOT, "include", "lesseq_hip.h")).read()
    assert "#define LSQ_ABI_VERSION 2" in header and L.lib.lsq_abi_version() == 2
    declared = set(re.findall(r"\b(lsq_gtf_\w+|lsq_le_load_gtf)\s*\(", header))
    assert {"lsq_gtf_parse", "lsq_gtf_parse_text", "lsq_gtf_free", "lsq_gtf_num_transcripts", "lsq_gtf_num_genes", "lsq_gtf_transcript_name",
            "lsq_gtf_transcript_chrom", "lsq_gtf_transcript_strand", "lsq_gtf_transcript_exons", "lsq_gtf_format", "lsq_gtf_result_times",
            "lsq_gtf_isoform_map", "lsq_le_load_gtf"} <= declared
    for name in declared:
        assert hasattr(L.lib, name), name
    assert "Annotation from GTF" in header


def test_argument_errors(tmp_path):
    out = C.c_void_p()
    assert L.lib.lsq_gtf_isoform_map(None, 3, C.byref(out)) == -1
    assert L.lib.lsq_gtf_isoform_map(b"a|b", 3, None) == -1
    assert L.lib.lsq_gtf_parse(None, b"x", C.byref(out)) == -1 and L.lib.lsq_gtf_parse_text(None, b"", 0, C.byref(out)) == -1
    assert L.lib.lsq_le_load_gtf(None, b"x", C.byref(out)) == -1
    assert L.lib.lsq_gtf_num_transcripts(None) == 0 and L.lib.lsq_gtf_transcript_name(None, 0) is None
    assert L.lib.lsq_gtf_transcript_exons(None, 0, None, None) == -1
    L.lib.lsq_gtf_free(None)
    # usage and unreadable input are reported before any GPU call
    for tool in ("parseGencode", "gencodeIsoformMap"):
        rc, text = L.cli_run(tool, ["a", "b"])
        assert rc == 1 and text == ""
        p = subprocess.run([os.path.join(BIN, tool), "a", "b"], capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and p.stdout == "" and "Usage" in p.stderr and tool in p.stderr
    rc, text = L.cli_run("gencodeIsoformMap", [str(tmp_path / "missing")])
    assert rc == 1 and text == ""
    p = subprocess.run([os.path.join(BIN, "events"), "--gtf", "only_one"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "events --gtf <gtf_path> <out_prefix>" in p.stderr
