"""Host-only test of stage 03's rows (`classify_read --rows device`): the integer rule of hast_amd/csrc/rr_core.h that prints a density
as printf("%0.6f") does, against glibc's snprintf inside tests/native/test_rr_core.cpp and against Python's own "%0.6f" here, and the
rows of every file of tests/rs_corpus.py against the restatement of tests/rr_model.py.  The program is stand-alone and runs once
plain and once under ASan + UBSan."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

from tests import rr_model as rr
from tests import rs_corpus as rc
from tests.conftest import ROOT
from tests.test_rb_core_cpu import make_votes

FMT = {rc.FASTA: "fasta", rc.FASTQ: "fastq"}
TOTALS = ((40, 37), (128, 37))                                    # 128: votes over a power of two print ties (1/128 = 0.0078125)
N_RANDOM, SEED = 3000000, 5
EXTREMES = ((2 ** 32 - 1, 1), (1, 2 ** 32 - 1), (2 ** 32 - 1, 2 ** 32 - 1), (1, 1), (2 ** 32 - 2, 2 ** 32 - 1), (1, 2 ** 31), (2 ** 32 - 1, 2),
            (999999, 1000000), (9999995, 10000000), (1, 2000000), (3, 2000000), (1, 128), (3, 128))


def build_native(out_dir, sanitize=False):
    """tests/native/test_rr_core.cpp as a stand-alone program, optionally under ASan + UBSan"""
    out = os.path.join(str(out_dir), "test_rr_core_san" if sanitize else "test_rr_core")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra"] + (["-fsanitize=address,undefined"] if sanitize else []) + \
          ["-o", out, os.path.join(ROOT, "tests", "native", "test_rr_core.cpp")]
    subprocess.run(cmd, check=True)
    return out


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("rr_core")


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def driver(request, work):
    return build_native(work, sanitize=request.param == "asan_ubsan")


@pytest.fixture(scope="module")
def plain_driver(work):
    return build_native(work)


def check(r):
    assert r.returncode == 0 and b"runtime error" not in r.stderr and b"Sanitizer" not in r.stderr, r.stderr.decode()[-2000:]


def test_the_density_is_what_snprintf_prints(driver):
    """every v, t in 1..3000; v in 1..200 000 over every t = 2^k; the extremes; random 32-bit pairs: the text, row_bytes, and q against
    exact 128-bit arithmetic, all inside the program.  Ties must have been met both ways."""
    r = subprocess.run([driver, "-s", str(N_RANDOM), str(SEED)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    check(r)
    m = re.fullmatch(rb"cases (\d+) diffs (\d+) ties_down (\d+) ties_up (\d+)\n", r.stdout)
    assert m, r.stdout
    cases, diffs, down, up = (int(x) for x in m.groups())
    assert cases == 3000 * 3000 + 32 * 200000 + len(EXTREMES) + N_RANDOM and diffs == 0
    assert down > 1000 and up > 1000, (down, up)


@pytest.mark.parametrize("cases", ("grid", "ties", "extremes", "rand"))
def test_the_density_is_what_python_prints(plain_driver, cases):
    if cases == "grid":
        v, t = np.tile(np.arange(1, 3001), 3000), np.repeat(np.arange(1, 3001), 3000)
    elif cases == "ties":
        v, t = np.tile(np.arange(1, 200001), 32), np.repeat(2 ** np.arange(32, dtype=np.int64), 200000)
    elif cases == "extremes":
        v, t = np.array([e[0] for e in EXTREMES]), np.array([e[1] for e in EXTREMES])
    else:
        v, t = rr.splitmix64_pairs(N_RANDOM, SEED)
    r = subprocess.run([plain_driver, "-D", cases] + ([str(N_RANDOM), str(SEED)] if cases == "rand" else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600)
    check(r)
    want = rr.density_lines(v, t)
    if r.stdout != want:
        got, exp = r.stdout.split(b"\n"), want.split(b"\n")
        bad = [(int(v[i]), int(t[i]), g, e) for i, (g, e) in enumerate(zip(got, exp)) if g != e]
        assert not bad and len(got) == len(exp), (bad[:5], len(got), len(exp))
    if cases == "extremes":
        assert r.stdout.split(b"\n")[:3] == [b"4294967295.000000", b"0.000000", b"1.000000"] and r.stdout.endswith(b"0.007812\n0.023438\n")
    if cases == "ties":                                           # odd v over 128 = x.xxxxxx5 exactly: a tie down, and one up
        lines = r.stdout.split(b"\n")
        assert lines[7 * 200000] == b"0.007812" and lines[7 * 200000 + 2] == b"0.023438"


@pytest.fixture(scope="module")
def corpus(work):
    """every file, votes for its records, and per pair of totals the model's rows"""
    rng = random.Random(78)
    out = []
    for name, fmt, data in rc.corpus(rc.make_keys(3, 21)):
        p = work / name
        p.write_bytes(data)
        want = rc.read_file(fmt, data)
        votes = make_votes(rng, 2000 if want == rc.ERR else len(want))
        (work / (name + ".votes")).write_bytes(votes.tobytes())
        out.append((name, fmt, str(p), data, want, votes))
    return out


@pytest.mark.parametrize("totals", TOTALS)
@pytest.mark.parametrize("fmt", (rc.FASTA, rc.FASTQ))
def test_the_rows_of_the_corpus_are_the_python_models(driver, corpus, fmt, totals):
    use = [c for c in corpus if c[1] == fmt]
    r = subprocess.run([driver, "-f", FMT[fmt], "-t", "%d,%d" % totals] + [c[2] for c in use], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    check(r)
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(use)
    seen, ties = [0, 0, 0], 0
    for (name, _, path, data, want, votes), line in zip(use, lines):
        f = line.split(" : ")[0].split()
        got = open(path + ".rows", "rb").read()
        if want == rc.ERR:
            assert f[0] == "format_error" and got == b"", (name, line)
            continue
        text, count, sizes = rr.file_rows(fmt, data, votes, *totals)
        assert f[0] == "ok", (name, line)                         # (the program has held its rows against format_rows of rr_host.h)
        assert [int(x) for x in f[1:4]] == count and int(f[4]) == len(want) and int(f[5]) == len(text) == sum(sizes), (name, line)
        assert got == text, (name, len(got), len(text))
        for c in range(3):
            seen[c] += count[c]
        ties += sum(1 for v0, v1 in votes[:len(want)] if totals[0] == 128 and v0 % 2 == 1 and rr.row(b"", int(v0), int(v1), *totals)[1] == 0)
    assert min(seen) > 50
    assert ties > 20 or totals[0] != 128
