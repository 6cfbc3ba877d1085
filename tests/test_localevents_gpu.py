"""events on the device: Events.r's eight local-event annotations, checked against literal lines worked out by hand from
the script, against the Python restatement in localev_ref.py on every golden classify/ directory and on generated gene
models (N, K > 64 included), annotation mode against classify + drop-in mode byte for byte, append behaviour, both
forms of the executable, and the annotation through count / solve against the oracle."""
import os
import random
import subprocess

import pytest

import lesseq_amd as L
from lesseq_amd import localevents as le
import golden_inputs as gi
import localev_ref as R
import oracle_binding as ob

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
BIN = os.path.join(os.path.dirname(HERE), "lesseq_amd", "bin")


def _classify(iv, mp, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    rc, _ = L.cli_run("classify", ["0", "x", out_dir + "/", "LH_GENE_TXT", iv, "UCSC_GENE2ISOFORM", mp, "0", "100000000"])
    assert rc == 0


def _dropin(prefix, group, out_prefix):
    rc, text = L.cli_run("events", [prefix, group, out_prefix])
    return rc, text


def _annot(iv, mp, out_prefix):
    return L.cli_run("events", ["--annotation", "LH_GENE_TXT", iv, "UCSC_GENE2ISOFORM", mp, out_prefix])


def test_toy_literal_lines(tmp_path):
    d = os.path.join(GOLD, "toy")
    rc, text = _dropin(os.path.join(d, "classify") + "/", os.path.join(d, "toy.map"), str(tmp_path) + "/")
    assert rc == 0
    assert text == '[1] "processing gene: RI1"\n[1] "processing gene: SE1"\n'
    assert sorted(os.listdir(tmp_path)) == ["ES.interval", "ES.map", "RI.interval", "RI.map"]
    assert open(tmp_path / "ES.interval").read() == (
        "SE1|2|1\tchr1\t+\t1000\t1600\t3\t1000,1200,1500\t1100,1300,1600\n"
        "SE1|2|2\tchr1\t+\t1000\t1600\t2\t1000,1500\t1100,1600\n")
    assert open(tmp_path / "ES.map").read() == "1\tSE1|2|1\n1\tSE1|2|2\n"
    assert open(tmp_path / "RI.interval").read() == (
        "RI1|2|1\tchr1\t+\t5000\t5500\t3\t5000,5200,5300\t5200,5300,5500\n"
        "RI1|2|2\tchr1\t+\t5000\t5500\t2\t5000,5300\t5200,5500\n")
    assert open(tmp_path / "RI.map").read() == "1\tRI1|2|1\n1\tRI1|2|2\n"


# every golden classify/ directory; the map is cut to the genes classify wrote (events_s2 was classified over a range of
# genes), where Events.r reads without stopping.  (classify_mix: cut has two map lines but no matrix; the next test.)
GOLDEN = [("toy", "toy.map"), ("events_s1", "ev.map"), ("events_s2", "ev.map"), ("events_s3", "ev.map"), ("wide", "wide.map")]


@pytest.mark.parametrize("name,grp", GOLDEN)
def test_golden_matches_restatement(name, grp, tmp_path, gpu_ctx):
    d = os.path.join(GOLD, name)
    prefix = os.path.join(d, "classify") + "/"
    have = {fn[:-len(".matrix")] for fn in os.listdir(prefix)}
    lines = [ln for ln in open(os.path.join(d, grp)).read().splitlines() if ln.split("\t")[0] in have]
    group = str(tmp_path / "group.map")
    open(group, "w").write("\n".join(lines) + "\n")
    (tmp_path / "out").mkdir()
    tmp_path = tmp_path / "out"
    want_out, want = R.events_files(prefix, group)
    rc, text = _dropin(prefix, group, str(tmp_path) + "/")
    assert rc == 0 and text == want_out
    assert R.read_out(str(tmp_path) + "/") == want
    # the Python module gives the same records
    res = le.Graphs.from_matrices(prefix, group).detect(gpu_ctx)
    recs = res.records()
    for t in le.TYPES:
        lines = want.get(t + ".interval", "").splitlines()
        assert [r.id for r in recs[t]] == [ln.split("\t")[0] for ln in lines]
        maps = want.get(t + ".map", "").splitlines()
        assert [r.counter for r in recs[t]] == [ln.split("\t")[0] for ln in maps]


@pytest.mark.parametrize("name,iv,mp", [("toy", "toy.interval", "toy.map"), ("events_s1", "ev.interval", "ev.map"),
                                        ("events_s2", "ev.interval", "ev.map"), ("events_s3", "ev.interval", "ev.map"),
                                        ("wide", "wide.interval", "wide.map")])
def test_annotation_mode_equals_classify_then_dropin(name, iv, mp, tmp_path):
    d = os.path.join(GOLD, name)
    iv, mp = os.path.join(d, iv), os.path.join(d, mp)
    _classify(iv, mp, str(tmp_path / "cls"))
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    rc1, t1 = _dropin(str(tmp_path / "cls") + "/", mp, str(tmp_path / "a") + "/ev_")
    rc2, t2 = _annot(iv, mp, str(tmp_path / "b") + "/ev_")
    assert rc1 == rc2 == 0 and t1 == t2
    assert R.read_out(str(tmp_path / "a") + "/ev_") == R.read_out(str(tmp_path / "b") + "/ev_")


def test_classify_mix_annotation_mode_succeeds(tmp_path):
    d = os.path.join(GOLD, "classify_mix")
    rc, _ = _dropin(os.path.join(d, "classify") + "/", os.path.join(d, "cm.map"), str(tmp_path) + "/ev_")
    assert rc == 1
    rc, text = _annot(os.path.join(d, "cm.interval"), os.path.join(d, "cm.map"), str(tmp_path) + "/ev_")
    assert rc == 0
    assert text == '[1] "processing gene: far"\n[1] "processing gene: tri"\n'


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gen"))
    genes = R.gene_models(32000, seed=11, wide_every=1500)
    iv, mp = R.write_models(genes, d, "gen")
    _classify(iv, mp, os.path.join(d, "cls"))
    return d, iv, mp, genes


def test_generated_matches_restatement(generated, tmp_path):
    d, iv, mp, genes = generated
    prefix = os.path.join(d, "cls") + "/"
    want_out, want = R.events_files(prefix, mp)
    assert want["ES.map"].count("\n") // 2 >= 100000
    shapes = [R.read_matrix(prefix + g + ".matrix") for g, _ in genes[:3000]]
    assert {s[1] for s in shapes} == {"+", "-", "."}
    assert any(len(s[3][0]) == 3 for s in shapes) and any(len(s[3][0]) == 4 for s in shapes)
    assert any(len(s[3][0]) > 64 for s in shapes) and any(len(s[3]) > 64 for s in shapes)
    for t in le.TYPES:
        assert t + ".map" in want, t
    rc, text = _dropin(prefix, mp, str(tmp_path) + "/ev_")
    assert rc == 0 and text == want_out
    assert R.read_out(str(tmp_path) + "/ev_") == want
    (tmp_path / "b").mkdir()
    rc, text2 = _annot(iv, mp, str(tmp_path / "b") + "/ev_")
    assert rc == 0 and text2 == want_out
    assert R.read_out(str(tmp_path / "b") + "/ev_") == want


def test_hand_written_shapes(tmp_path):
    """ncol < 3 printed and skipped; no MXE at N = 3; one isoform row; strand '.' gives ES but no A5SS / T3"""
    m = tmp_path / "m"
    m.mkdir()

    def mat(name, header, rows):
        (m / (name + ".matrix")).write_text(header + "\n" + "".join("".join("%d\t" % v for v in r) + "\n" for r in rows))
    mat("a", "c\t+\t[1,2)-[3,4)-", [[1, 1], [1, 0]])
    mat("b", "c\t+\t[10,20)-[30,40)-[50,60)-", [[1, 0, 1], [0, 1, 0]])       # complement pair, N = 3
    mat("c", "c\t+\t[10,20)-[30,40)-[50,60)-", [[1, 0, 1]])                  # one row: usage 1, 0, 1
    mat("d", "c\t.\t[10,20)-[20,40)-[50,60)-[60,70)-", [[1, 1, 1, 1], [1, 0, 1, 0]])
    (tmp_path / "g").write_text("".join("%s\t1\n%s\t2\n" % (x, x) for x in "abcd"))
    want_out, want = R.events_files(str(m) + "/", str(tmp_path / "g"))
    rc, text = _dropin(str(m) + "/", str(tmp_path / "g"), str(tmp_path) + "/o_")
    assert rc == 0 and text == want_out and text.count("\n") == 4
    got = R.read_out(str(tmp_path) + "/o_")
    assert got == want
    assert "MXE.interval" not in got
    assert "c|2|1" in got["ES.interval"] and "d|2|1" not in got.get("A5SS.interval", "")


def test_append_and_no_empty_file(tmp_path):
    d = os.path.join(GOLD, "toy")
    args = (os.path.join(d, "classify") + "/", os.path.join(d, "toy.map"), str(tmp_path) + "/")
    assert _dropin(*args)[0] == 0
    assert _dropin(*args)[0] == 0
    assert sorted(os.listdir(tmp_path)) == ["ES.interval", "ES.map", "RI.interval", "RI.map"]
    assert open(tmp_path / "ES.map").read() == "1\tSE1|2|1\n1\tSE1|2|2\n" * 2     # counter restarts at 1
    assert open(tmp_path / "ES.interval").read().count("\n") == 4


def test_process_cli_both_forms(tmp_path):
    d = os.path.join(GOLD, "wide")
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    p1 = subprocess.run([os.path.join(BIN, "events"), "classify/", "wide.map", str(tmp_path / "a") + "/"], cwd=d,
                        capture_output=True, text=True, timeout=120)
    p2 = subprocess.run([os.path.join(BIN, "events"), "--annotation", "LH_GENE_TXT", "wide.interval", "UCSC_GENE2ISOFORM",
                         "wide.map", str(tmp_path / "b") + "/"], cwd=d, capture_output=True, text=True, timeout=120)
    assert p1.returncode == 0 and p2.returncode == 0, (p1.stderr, p2.stderr)
    assert p1.stdout == p2.stdout == R.events_files(os.path.join(d, "classify") + "/", os.path.join(d, "wide.map"))[0]
    assert R.read_out(str(tmp_path / "a") + "/") == R.read_out(str(tmp_path / "b") + "/")
    p3 = subprocess.run([os.path.join(BIN, "events"), "classify/"], cwd=d, capture_output=True, text=True, timeout=60)
    assert p3.returncode == 1 and "Usage" in p3.stderr


def test_pipeline_events_count_solve_against_oracle(tmp_path):
    """gene models -> events --annotation -> reads over the event forms -> count / solve, against the oracle (ES, MXE)"""
    genes = R.gene_models(400, seed=5, wide_every=0)
    iv, mp = R.write_models(genes, str(tmp_path), "g")
    rc, _ = _annot(iv, mp, str(tmp_path) + "/ev_")
    assert rc == 0
    rng = random.Random(9)
    for t in ("ES", "MXE"):
        ivp, mpp = str(tmp_path / ("ev_%s.interval" % t)), str(tmp_path / ("ev_%s.map" % t))
        forms = []
        for ln in open(ivp):
            f = ln.rstrip("\n").split("\t")
            forms.append((f[1], f[2], list(zip(map(int, f[6].split(",")), map(int, f[7].split(","))))))
        lines = ["AlignmentBlocks\n"]
        for _ in range(6000):
            chrom, strand, exons = forms[rng.randrange(len(forms))]
            L_ = sum(e - s for s, e in exons)
            if L_ < 40:
                continue
            st = rng.randrange(0, L_ - 40 + 1)
            lines.append(gi.mrf_line(chrom, strand, gi.transcript_blocks(exons, st, 40)))
        mrf = str(tmp_path / ("%s.mrf" % t))
        open(mrf, "w").writelines(lines)
        argv = ["0", t, "./", "LH_GENE_TXT", ivp, "UCSC_GENE2ISOFORM", mpp, "0", "1000000", "MRF_SINGLE", "SHORT_READ", "40", mrf]
        rc, text = L.cli_run("count", argv)
        orc, otext, _ = ob.run("count", argv)
        assert rc == 0 and orc == 0 and text == otext
        rc, text = L.cli_run("solve", argv + ["240000"])
        orc, otext, _ = ob.run("solve", argv + ["240000"])
        assert rc == 0 and orc == 0 and ob.solve_text_close(text, otext)
