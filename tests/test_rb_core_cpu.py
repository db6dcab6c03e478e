"""Host-only test of the read bins of `classify_read --bin-reads`: the class rule of hast_amd/csrc/rb_core.h, and the three runs of
the host model (rb_host.h, stepped view by view in tests/native/test_rb_core.cpp) against an independent restatement in Python
(tests/rb_model.py) over every file of tests/rs_corpus.py, once plain and once under ASan + UBSan."""
import os
import random
import subprocess

import numpy as np
import pytest

from tests import rb_model as rb
from tests import rs_corpus as rc
from tests.conftest import ROOT

BLOCKS = (64, 700, 4096)
FMT = {rc.FASTA: "fasta", rc.FASTQ: "fastq"}
T0, T1 = 40, 37                                                   # set sizes that differ: d1 > d0 is not v1 > v0


def build_native(out_dir, sanitize=False):
    """tests/native/test_rb_core.cpp as a stand-alone program, optionally under ASan + UBSan"""
    out = os.path.join(str(out_dir), "test_rb_core_san" if sanitize else "test_rb_core")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra"] + (["-fsanitize=address,undefined"] if sanitize else []) + \
          ["-o", out, os.path.join(ROOT, "tests", "native", "test_rb_core.cpp")]
    subprocess.run(cmd, check=True)
    return out


def make_votes(rng, n):
    """n pairs: zeros, ties, one-sided, and pairs around the line v1 / T1 = v0 / T0"""
    out = np.zeros((n, 2), dtype=np.uint32)
    for i in range(n):
        kind = rng.randrange(6)
        a = rng.randint(1, 60)
        out[i] = ((0, 0), (a, a), (a, 0), (0, a), (a, max(0, a - 1)), (rng.randint(0, 60), rng.randint(0, 60)))[kind]
    return out


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("rb_core")


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def driver(request, work):
    return build_native(work, sanitize=request.param == "asan_ubsan")


@pytest.fixture(scope="module")
def corpus(work):
    """every file with the reference reader's records, votes for them, and the model's runs"""
    rng = random.Random(77)
    out = []
    for name, fmt, data in rc.corpus(rc.make_keys(3, 21)):
        p = work / name
        p.write_bytes(data)
        want = rc.read_file(fmt, data)
        votes = make_votes(rng, 2000 if want == rc.ERR else len(want))       # (a format error may show only views later: votes for those in front)
        (work / (name + ".votes")).write_bytes(votes.tobytes())
        out.append((name, fmt, str(p), data, want, votes, None if want == rc.ERR else rb.runs(fmt, data, votes, T0, T1)))
    return out


def check(r):
    assert r.returncode == 0 and b"runtime error" not in r.stderr and b"Sanitizer" not in r.stderr, r.stderr.decode()[-2000:]


CLASS_CASES = [
    # v0, v1, t0, t1 -> class
    ((0, 0, 40, 37), 2), ((0, 0, 0, 0), 2), ((0, 0, 0, 37), 2),
    ((5, 5, 40, 40), 0), ((5, 5, 40, 37), 1), ((5, 5, 37, 40), 0),           # a tie in votes is one in densities only for equal sets
    ((1, 0, 40, 37), 0), ((0, 1, 40, 37), 1),
    ((38, 36, 40, 37), 1), ((36, 38, 37, 40), 0),                            # d1 > d0 against v1 > v0, both ways
    ((40, 37, 40, 37), 0), ((37, 40, 37, 40), 0),                            # both densities 1.0: haplotype0
    ((1, 0, 0, 37), 0), ((0, 1, 40, 0), 1), ((1, 1, 0, 0), 0), ((1, 2, 0, 0), 0),   # inf: never above inf
    ((0, 1, 0, 37), 0), ((1, 0, 40, 0), 0), ((0, 1, 0, 0), 0),               # NaN on one side: not above 0, and nothing is above it
    ((7, 1, 0, 37), 0), ((1, 7, 0, 37), 0),                                  # inf against a finite density
    ((2 ** 32 - 1, 2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32 - 1), 0), ((2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1), 1),
    ((2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 2), 1), ((2 ** 32 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 31), 0),
    ((2 ** 32 - 1, 1, 2 ** 32 - 1, 1), 0), ((2 ** 32 - 2, 1, 2 ** 32 - 1, 1), 1),
]


def test_the_class_rule(driver):
    rng = random.Random(9)
    cases = [c for c, _ in CLASS_CASES]
    for _ in range(3000):
        t0, t1 = rng.choice((0, 1, 37, 40, 2 ** 32 - 1)), rng.choice((0, 1, 37, 40, 2 ** 32 - 1))
        hi = rng.choice((3, 60, 2 ** 32 - 1))
        cases.append((rng.randint(0, hi), rng.randint(0, hi), t0, t1))
    text = "".join("%d %d %d %d\n" % c for c in cases).encode()
    r = subprocess.run([driver, "-c"], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    check(r)
    got = [int(x) for x in r.stdout.split()]
    assert len(got) == len(cases)
    for (c, want), g in zip(CLASS_CASES, got):
        assert g == want and rb.read_class(*c) == want, (c, g, want)
    bad = [(c, g) for c, g in zip(cases, got) if g != rb.read_class(*c)]
    assert not bad, bad[:5]
    assert any(rb.read_class(*c) == 1 and c[1] < c[0] for c in cases) and any(rb.read_class(*c) == 0 and c[1] > c[0] for c in cases)
    assert {0, 1, 2} == set(got)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("fmt", (rc.FASTA, rc.FASTQ))
def test_the_host_models_runs_are_the_python_models(driver, corpus, fmt, block):
    use = [c for c in corpus if c[1] == fmt]
    r = subprocess.run([driver, "-f", FMT[fmt], "-b", str(block), "-t", "%d,%d" % (T0, T1)] + [c[2] for c in use], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    check(r)
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(use)
    seen = [0, 0, 0]
    for (name, _, path, data, want, votes, model), line in zip(use, lines):
        f = line.split(" : ")[0].split()
        got = [open("%s.bin%d" % (path, c), "rb").read() for c in range(3)]
        if want == rc.ERR:
            assert f[0] == "format_error" and got == [b"", b"", b""], (name, block, line)
            continue
        runs, count, _ = model
        assert f[0] == "ok", (name, block, line)
        assert [int(x) for x in f[1:4]] == count and int(f[4]) == len(want), (name, block, line)
        assert int(f[5]) == -(-len(data) // block) + 1, (name, block, line)
        for c in range(3):
            assert got[c] == runs[c], (name, block, c, len(got[c]), len(runs[c]))
            seen[c] += count[c]
    assert min(seen) > 50


def test_the_python_model_frames_what_the_reference_reader_frames(corpus):
    """the restated extents against the restated reader: as many records, every extent opens with its record's header line and its
    other lines, joined, are the record's sequence (FASTA) or start with it (FASTQ); what no extent holds is junk, or a cut-off end"""
    n_votes_disagree = 0
    for name, fmt, _, data, want, votes, model in corpus:
        if want == rc.ERR:
            continue
        ext = rb.extents(fmt, data)
        assert len(ext) == len(want), name
        for e, (rname, seq) in zip(ext, want):
            lines = e.split(b"\n")
            assert e.endswith(b"\n") and lines[0][1:] == rname, name
            if fmt == rc.FASTA:
                assert lines[0][:1] == b">" and b"".join(lines[1:]) == seq, name
            else:
                assert lines[1] == seq and e.count(b"\n") <= 4, name
        joined = b"".join(ext)
        if fmt == rc.FASTQ:
            assert joined == data[:len(joined)] or joined == data + b"\n", name
        else:
            assert joined in data and (not ext or data.index(joined) == data.index(ext[0])), name
        n_votes_disagree += sum(1 for c, (v0, v1) in zip(model[2], votes) if c != (2 if v0 == v1 == 0 else 1 if v1 > v0 else 0))
    assert n_votes_disagree > 100
