"""The argv of count / solve as the executables read it before any device is touched: the `--fim`, `--bootstrap` and `--seed`
extensions and their quirks, the log level that fails the cast, numbers that fail it, too many read files, the tool an
executable's name chooses, a tool nobody knows.  Every case ends before the annotation is opened: no GPU."""
import os
import shutil
import subprocess

import pytest

import lesseq_amd as L
from test_oracle_golden import load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lesseq_amd", "bin")
LEXICAL = "Lexical_cast error when converting arguments to numeric values"
MAX_METHODS = 8         # LSQ_MAX_METHODS of include/lesseq_hip.h


def changed(argv, at, word):
    return argv[:at] + [word] + argv[at + 1:]


def rows(c):
    """(tool, argv, exit status, what standard error holds, what it does not hold)"""
    count, solve = c["count"][0]["argv"], c["solve"][0]["argv"]
    group = ["MRF_SINGLE", "SHORT_READ", "50", "toy.mrf"]
    out = [("solve", solve + tail.split(), 1, "Usage:\nsolve\n", LEXICAL) for tail in (
        "--bootstrap 0", "--bootstrap 4097", "--bootstrap x", "--bootstrap 10 --seed", "--bootstrap 10 --sed 3",
        "--bootstrap 10 --seed x", "--bootstrap 10 --fim")]
    out.append(("count", count + ["--fim"], 1, "Usage:\ncount\n", LEXICAL))           # the start of an incomplete file group
    out.append(("count", changed(count, 0, "abc"), 134, "", "ERROR"))                 # lexical_cast outside the try block
    out.append(("count", changed(count, 7, "abc"), 1, LEXICAL, "Usage"))
    out.append(("count", changed(count, 11, "fifty"), 1, LEXICAL, "Usage"))
    out.append(("solve", changed(solve, 13, "abc"), 1, LEXICAL, "Usage"))
    out.append(("count", count[:9] + group * (MAX_METHODS + 1), 2, "more than %d read files" % MAX_METHODS, "Usage"))
    out.append(("solve", solve[:9] + (group + ["650"]) * (MAX_METHODS + 1), 2, "more than %d read files" % MAX_METHODS, "Usage"))
    return out


N_ROWS = 14


@pytest.mark.parametrize("k", range(N_ROWS))
def test_argv_decided_before_anything_is_opened(k, tmp_path, monkeypatch, capfd):
    c, d = load_case("toy", tmp_path)
    assert len(rows(c)) == N_ROWS
    tool, argv, status, holds, lacks = rows(c)[k]
    monkeypatch.chdir(d)
    capfd.readouterr()
    rc, text = L.cli_run(tool, argv)
    err = capfd.readouterr().err
    assert rc == status and text == "", (tool, argv, rc, err)
    assert holds in err and lacks not in err, (tool, argv, err)
    assert ("ERROR" in err) == (status != 134)


@pytest.mark.parametrize("k", (0, 8, 11))
def test_argv_decided_before_anything_is_opened_as_processes(k, tmp_path):
    c, d = load_case("toy", tmp_path)
    tool, argv, status, holds, lacks = rows(c)[k]
    p = subprocess.run([os.path.join(BIN, tool)] + argv, cwd=d, capture_output=True, text=True)
    assert p.returncode == status and p.stdout == "", (tool, argv, p.returncode, p.stderr)
    assert holds in p.stderr and lacks not in p.stderr, (tool, argv, p.stderr)


def test_the_tool_is_a_substring_of_the_program_name(tmp_path):
    """bin/solve under the name xsolve-1 is still solve: the usage text it prints says so"""
    c, d = load_case("toy", tmp_path)
    exe = str(tmp_path / "xsolve-1")
    shutil.copy(os.path.join(BIN, "solve"), exe)
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "lesseq_amd", "_build") + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    p = subprocess.run([exe] + c["solve"][0]["argv"] + ["--bootstrap", "0"], cwd=d, capture_output=True, text=True, env=env)
    assert p.returncode == 1 and p.stdout == "" and "Usage:\nsolve\n" in p.stderr and "total_read_bases" in p.stderr, (p.returncode, p.stderr)
    # ... and a name that holds no tool's is count
    other = str(tmp_path / "tool")
    shutil.copy(os.path.join(BIN, "solve"), other)
    p = subprocess.run([other], cwd=d, capture_output=True, text=True, env=env)
    assert p.returncode == 1 and p.stdout == "" and "Usage:\ncount\n" in p.stderr, (p.returncode, p.stderr)


def test_a_tool_nobody_knows(tmp_path, monkeypatch):
    c, d = load_case("toy", tmp_path)
    monkeypatch.chdir(d)
    rc, text = L.cli_run("nonesuch", c["count"][0]["argv"])
    assert rc == 2 and text == ""
