"""SAM_SINGLE on the device: the SAM routing kernels (lsq_sam_device.hpp) against the host parser, and count / solve from
SAM text against the reference's stdout on the equivalent MRF (tests/golden/sam, made by tools/make_sam_golden.py).
Need an MI355X: python -m pytest tests -m gpu.  Every case directory is run; none is skipped."""
import os
import subprocess

import numpy as np
import pytest

import lesseq_amd as L
import oracle_binding as ob
from test_sam_host import GOLD, BIN, SAM_CASES, BAD_LINES, LSQ_E_PARSE, GOOD, load, read, same_reads, events_of, bad_file

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 300      # seconds for one executable run


def test_every_case_directory_is_run():
    assert SAM_CASES == ["basic", "cigar", "filters", "multi", "names"]


def context_for(d, R=100, rtype="SHORT_READ"):
    ev = events_of(d, R, rtype)
    ctx = L.Context(0)
    ctx.upload_events(ev)
    return ev, ctx


@pytest.mark.parametrize("name", SAM_CASES)
def test_device_parser_equals_host_parser(name):
    c, d = load(name)
    for cv in c["conversions"]:
        ev, ctx = context_for(d)
        ctx.set_option("sam_skip_flags", cv["skip_flags"])
        ctx.set_option("sam_min_mapq", cv["min_mapq"])
        dev = ctx.parse_sam_device(os.path.join(d, cv["sam"]))
        same_reads(ev, L.Reads.from_sam(os.path.join(d, cv["sam"]), ev, cv["skip_flags"], cv["min_mapq"]), dev)
        same_reads(ev, L.Reads.from_mrf(os.path.join(d, cv["mrf"]), ev), dev)
        ctx.close()


@pytest.mark.parametrize("kind,line", BAD_LINES, ids=[k for k, _ in BAD_LINES])
def test_error_files_give_the_host_parsers_status_and_message(kind, line, tmp_path, monkeypatch):
    """the parse-device kernels, the tile kernel with its fall-back, and the byte-walking form: each reports the first malformed
    line in file order as the host parser does"""
    second = BAD_LINES[0][1] if kind != "five_fields" else BAD_LINES[3][1]
    text, k = bad_file(line, second)
    path = str(tmp_path / "bad.sam")
    with open(path, "w") as f:
        f.write(text)
    ev, ctx = context_for(os.path.join(GOLD, "cigar"), 50)
    with pytest.raises(L.LsqError) as host:
        L.Reads.from_sam(path, ev)
    assert host.value.status == LSQ_E_PARSE and str(host.value).endswith(": #%d:%s" % (k, line))
    with pytest.raises(L.LsqError) as e:
        ctx.parse_sam_device(path)
    assert (e.value.status, str(e.value)) == (host.value.status, str(host.value))
    with pytest.raises(L.LsqError) as e:
        ctx.upload_reads_sam(0, path)
    assert (e.value.status, str(e.value)) == (host.value.status, str(host.value))
    monkeypatch.setenv("LSQ_SAM_SLOW", "1")
    with pytest.raises(L.LsqError) as e:
        ctx.upload_reads_sam(0, path)
    assert (e.value.status, str(e.value)) == (host.value.status, str(host.value))
    ctx.close()


def check_run(name, r, rc, text, d):
    exp = open(os.path.join(d, r["stdout"])).read()
    assert rc == r["exit"], (name, r["argv"])
    if r["tool"] == "count":
        assert text == exp, (name, r["argv"], text, exp)
    else:
        assert ob.solve_text_close(text, exp), (name, r["argv"], text, exp)


def option_env(r):
    env = {}
    if "sam_skip_flags" in r["options"]:
        env["LSQ_SAM_SKIP_FLAGS"] = str(r["options"]["sam_skip_flags"])
    if "sam_min_mapq" in r["options"]:
        env["LSQ_SAM_MIN_MAPQ"] = str(r["options"]["sam_min_mapq"])
    return env


@pytest.mark.parametrize("name", SAM_CASES)
def test_count_and_solve_from_sam_match_the_reference(name, monkeypatch):
    """in-process: count byte for byte, solve as printed within one unit of the sixth digit, exit statuses equal; the
    non-default filters through the environment variables"""
    c, d = load(name)
    monkeypatch.chdir(d)
    n = 0
    for r in c["runs"]:
        for k in ("LSQ_SAM_SKIP_FLAGS", "LSQ_SAM_MIN_MAPQ"):
            monkeypatch.delenv(k, raising=False)
        for k, v in option_env(r).items():
            monkeypatch.setenv(k, v)
        rc, text = L.cli_run(r["tool"], r["argv"])
        check_run(name, r, rc, text, d)
        n += 1
    assert n == len(c["runs"]) and n >= 2


@pytest.mark.parametrize("name", SAM_CASES)
def test_executables_from_sam_match_the_reference(name):
    """once as child processes of the executables (the second thread stages the SAM text beside the annotation load)"""
    c, d = load(name)
    for r in c["runs"]:
        p = subprocess.run([os.path.join(BIN, r["tool"])] + r["argv"], cwd=d, capture_output=True, text=True, env=dict(os.environ, **option_env(r)), timeout=CHILD_TIMEOUT)
        check_run(name, r, p.returncode, p.stdout, d)


def count_table(ctx, ev):
    ctx.count()
    cnt, _ = ctx.counts()
    return L.format_count(ev, cnt)


def test_filter_options_through_set_option_give_the_filters_goldens():
    c, d = load("filters")
    seen = 0
    for r in c["runs"]:
        if r["tool"] != "count":
            continue
        ev, ctx = context_for(d)
        for k, v in r["options"].items():
            ctx.set_option(k, v)
        ctx.upload_reads_sam(0, os.path.join(d, "in.sam"))
        assert count_table(ctx, ev) == open(os.path.join(d, r["stdout"])).read(), r["options"]
        ctx.close()
        seen += 1
    assert seen == 3
    ev, ctx = context_for(d)
    for name, bad in (("sam_skip_flags", -1), ("sam_skip_flags", 65536), ("sam_min_mapq", -1), ("sam_min_mapq", 1000)):
        with pytest.raises(L.LsqError):
            ctx.set_option(name, bad)
    ctx.close()


def test_both_kernel_paths_against_the_host_parser(tmp_path, monkeypatch):
    """`basic`: every line settled by the tile kernel; `cigar`: its 300-operation CIGARs and its 300-byte QNAME go to the
    fall-back kernel; a file of long heads with no room on the list: every tile once more in the byte-walking form; and the
    byte-walking form asked for.  Each against the pools the host parser's arrays give."""
    def tables(ctx, ev):
        t = count_table(ctx, ev)
        return t, ctx.retained(0), ctx.pooled_blocks(0)

    for name, listed in (("basic", False), ("cigar", True)):
        c, d = load(name)
        R = int(c["runs"][0]["argv"][11])
        ev, ctx = context_for(d, R)
        ctx.upload_reads(0, L.Reads.from_sam(os.path.join(d, "in.sam"), ev))
        want = tables(ctx, ev)
        ctx.upload_reads_sam(0, os.path.join(d, "in.sam"))
        paths = ctx.sam_paths()
        assert not paths["whole_file_byte_walking"] and (paths["lines_to_fall_back_kernel"] > 0) == listed, paths
        if listed:
            assert paths["lines_to_fall_back_kernel"] >= 4
        assert tables(ctx, ev) == want
        assert [s["stage"] for s in ctx.ingest_stages()][:2] == ["newline_count", "sam_route"]
        monkeypatch.setenv("LSQ_SAM_SLOW", "1")
        ctx.upload_reads_sam(0, os.path.join(d, "in.sam"))
        assert ctx.sam_paths() == {"lines_to_fall_back_kernel": 0, "whole_file_byte_walking": True}
        assert tables(ctx, ev) == want
        monkeypatch.delenv("LSQ_SAM_SLOW")
        # an MRF ingest afterwards reports its own pass name again
        ctx.upload_reads_mrf(0, os.path.join(d, "in.mrf"))
        assert [s["stage"] for s in ctx.ingest_stages()][:2] == ["newline_count", "route"]
        assert tables(ctx, ev) == want
        ctx.close()
    # long heads everywhere and no room on the list
    c, d = load("cigar")
    lines = read(os.path.join(d, "in.sam")).decode("latin-1").split("\n")[:-1]
    recs = [ln for ln in lines if not ln.startswith("@") and len(ln) < 1000]
    text = "\n".join(("n" * 290 + ln) for ln in recs * 3) + "\n"
    path = str(tmp_path / "long_heads.sam")
    with open(path, "w", encoding="latin-1") as f:
        f.write(text)
    ev, ctx = context_for(d, 50)
    ctx.upload_reads(0, L.Reads.from_sam(path, ev))
    want = tables(ctx, ev)
    ctx.upload_reads_sam(0, path)
    assert ctx.sam_paths()["lines_to_fall_back_kernel"] == 3 * len(recs) and tables(ctx, ev) == want
    monkeypatch.setenv("LSQ_SAM_LINE_LIST", "0")
    ctx.upload_reads_sam(0, path)
    assert ctx.sam_paths()["whole_file_byte_walking"] and tables(ctx, ev) == want
    same_reads(ev, L.Reads.from_sam(path, ev), ctx.parse_sam_device(path))
    ctx.close()


def test_lines_on_every_tile_boundary(tmp_path):
    """records whose start, head and newline fall on, just ahead of and just behind a tile boundary; runs of very short lines
    (more lines in a tile than one round of the walk holds); a file that ends with the tile"""
    tile = 7680
    d = os.path.join(GOLD, "cigar")
    short = "q\t0\tchr1\t1101\t60\t50M"
    for shift in list(range(0, 40)) + [tile - len(GOOD) - 1 + k for k in range(-3, 4)]:
        pad = "@CO\t" + "x" * max(shift - 5, 0)
        body = [pad] + [GOOD] * 60 + ["@"] * 3000 + [short] * 500 + [GOOD] * 30
        text = "\n".join(body) + "\n"
        if shift == 7:
            text += GOOD                     # ... and a last line without a newline
        path = str(tmp_path / "b.sam")
        with open(path, "w") as f:
            f.write(text)
        ev, ctx = context_for(d, 50)
        same_reads(ev, L.Reads.from_sam(path, ev), ctx.parse_sam_device(path))
        ctx.upload_reads(0, L.Reads.from_sam(path, ev))
        want = (count_table(ctx, ev), ctx.retained(0))
        ctx.upload_reads_sam(0, path)
        assert (count_table(ctx, ev), ctx.retained(0)) == want and want[1] == 590
        ctx.close()
    # exactly one tile, exactly two tiles
    for n_tiles in (1, 2):
        body = (GOOD + "\n") * 20
        text = body + "@CO\t" + "y" * (n_tiles * tile - len(body) - 5) + "\n"
        assert len(text) == n_tiles * tile
        path = str(tmp_path / "t.sam")
        with open(path, "w") as f:
            f.write(text)
        ev, ctx = context_for(d, 50)
        same_reads(ev, L.Reads.from_sam(path, ev), ctx.parse_sam_device(path))
        ctx.upload_reads_sam(0, path)
        assert ctx.retained(0) == 20
        ctx.close()


def test_two_slices_print_the_reference_table():
    c, d = load("basic")
    env = dict(os.environ, LSQ_GPUS="2", LSQ_DEVICES="0,0", LSQ_GATHER="host")
    for r in c["runs"]:
        p = subprocess.run([os.path.join(BIN, r["tool"])] + r["argv"], cwd=d, capture_output=True, text=True, env=env, timeout=CHILD_TIMEOUT)
        assert p.returncode == 0, p.stderr
        check_run("basic", r, p.returncode, p.stdout, d)
    # LSQ_SHARD=reads takes MRF_SINGLE files only: a SAM job is sharded by events instead and prints the same table
    r = c["runs"][0]
    p = subprocess.run([os.path.join(BIN, r["tool"])] + r["argv"], cwd=d, capture_output=True, text=True, env=dict(env, LSQ_SHARD="reads"), timeout=CHILD_TIMEOUT)
    check_run("basic", r, p.returncode, p.stdout, d)


def test_mid_size_run_from_sam_and_from_its_mrf(tmp_path):
    """2 M reads over 5 k events, Zipf depth: count and solve from the SAM text and from sam2mrf's output of it -- two front ends
    of the same code -- give equal count tables, class counts and EM iteration counts, and bit-for-bit equal theta"""
    spec = L.SynthSpec(2026, 5000, 2000000, 100, 8, L.EVENT_TYPES, zipf=True)
    L.synth_write_sam(spec, str(tmp_path), "m")
    sam, mrf = str(tmp_path / "m.sam"), str(tmp_path / "m.mrf")
    with open(mrf, "wb") as out:
        p = subprocess.run([os.path.join(BIN, "sam2mrf"), sam], stdout=out, stderr=subprocess.PIPE, timeout=CHILD_TIMEOUT)
    assert p.returncode == 0, p.stderr
    ev = L.Events(L.Annotation(str(tmp_path / "m.interval"), str(tmp_path / "m.map"), 0, 10 ** 9), ("SHORT_READ",), (100,))
    got = []
    for upload, path in (("upload_reads_sam", sam), ("upload_reads_mrf", mrf)):
        ctx = L.Context(0)
        ctx.upload_events(ev)
        getattr(ctx, upload)(0, path)
        retained = ctx.retained(0)
        ctx.count()
        cnt, bases = ctx.counts()
        ctx.solve()
        theta, ll, iters, flags = ctx.solution()
        got.append((retained, cnt.copy(), bases.copy(), theta.copy(), ll.copy(), iters.copy(), L.format_count(ev, cnt),
                    L.format_solve(ev, cnt, bases, theta, ll, [2e8])))
        if upload == "upload_reads_sam":
            assert not ctx.sam_paths()["whole_file_byte_walking"]
        ctx.close()
    a, b = got
    assert a[0] == b[0] and a[0] > 1000000
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and int(a[1].sum()) > 1000000
    assert np.array_equal(a[5], b[5])
    assert a[3].tobytes() == b[3].tobytes() and a[4].tobytes() == b[4].tobytes()
    assert a[6] == b[6] and a[7] == b[7]
