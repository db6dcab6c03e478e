"""Host-only test of the rules of the stage-00 device ingest (hast_amd/csrc/sq_core.h, stepped by tests/native/test_sq_core.cpp the
way `unshared_kmers --ingest device` feeds a file): on strict four-line FASTQ the framed stream is the host parser's, byte for byte,
and nothing is refused; a damaged input is refused, or read exactly as the parser reads it."""
import os
import shutil
import subprocess

import pytest

from tests import sq_corpus as sc
from tests.conftest import GOLDEN

BLOCKS = (64, 100, 700, 4096, 65536, 1 << 24)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("sq_core")


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def driver(request, work):
    return sc.build_native(work, sanitize=request.param == "asan_ubsan")


@pytest.fixture(scope="module")
def parser_driver(work):
    return sc.build_parser_driver(work)


@pytest.fixture(scope="module")
def corpus(work, parser_driver):
    """the valid inputs as files, with what the host parser makes of each"""
    out = []
    for name, data, longest in sc.valid_corpus():
        p = work / (name + ".fq")
        p.write_bytes(data)
        r = subprocess.run([parser_driver, str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, (name, r.stderr)
        out.append((name, str(p), data, longest, r.stdout))
    return out


def run_driver(driver, block, paths):
    r = subprocess.run([driver, "-b", str(block)] + list(paths), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"runtime error" not in r.stderr and b"Sanitizer" not in r.stderr, r.stderr.decode()[-2000:]
    rows = []
    for line, p in zip(r.stdout.decode().splitlines(), paths):
        f = line.split(" : ")[0].split()
        rows.append(dict(status=f[0], records=int(f[1]), bases=int(f[2]), bytes=int(f[3]), blocks=int(f[4]), first_bad=int(f[5]),
                         stream=open(p + ".sq", "rb").read(), line=line))
    assert len(rows) == len(paths)
    return rows


@pytest.mark.parametrize("block", BLOCKS)
def test_valid_inputs_frame_to_the_parsers_stream(driver, corpus, block):
    use = [c for c in corpus if c[3] <= block]          # a block has room for the longest record
    assert use
    rows = run_driver(driver, block, [c[1] for c in use])
    for (name, _, data, _, want), row in zip(use, rows):
        assert row["status"] == "ok", (name, block, row["line"])          # never refused: the generator's condition
        assert row["stream"] == want, (name, block)
        assert row["bytes"] == len(data) and row["records"] == want.count(b"\n") and row["bases"] == len(want) - want.count(b"\n"), (name, row["line"])
        if len(data) > 2 * block:
            assert row["blocks"] > 1, name


def test_every_read_length_and_count_is_in_the_corpus(corpus):
    names = {c[0] for c in corpus}
    for b in range(len(sc.BREAKS)):
        assert all("len%d_b%d" % (length, b) in names for length in sc.READ_LENS)
        assert all("n%d_b%d_%s" % (n, b, e) in names for n in sc.COUNTS for e in ("nl", "nonl"))
    assert any(b"\n@" in c[2].replace(b"\n@r", b"") for c in corpus) and any(b"\n+\n+" in c[2] or b"\n+\r\n+" in c[2] for c in corpus)
    assert any(b"a" in c[2] and b"N" in c[2] for c in corpus)


@pytest.mark.parametrize("block", (700, 65536))
def test_mutants_are_refused_or_read_as_the_parser_reads_them(driver, parser_driver, work, block):
    paths, kinds = [], []
    for last in (True, False):
        base = sc.fastq(31 + last, 40, (20, 0, 1, 64, 150, 7), b"\n", last)
        for kind in sc.MUTANTS:
            for seed in range(6):
                p = work / ("mut_%s_%d_%d.fq" % (kind, seed, last))
                p.write_bytes(sc.mutate(base, kind, seed))
                paths.append(str(p))
                kinds.append(kind)
    rows = run_driver(driver, block, paths)
    refused = 0
    for p, kind, row in zip(paths, kinds, rows):
        r = subprocess.run([parser_driver, p], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        if row["status"] == "ok":                       # taken: then the parser takes it too, and reads the same
            assert r.returncode == 0 and row["stream"] == r.stdout, (p, row["line"], r.stderr)
        else:                                           # refused: the program reads it with the host parser instead
            assert row["status"] in ("flagged", "badfirst", "tail") and row["stream"] == b"", (p, row["line"])
            if row["status"] == "flagged":
                assert row["first_bad"] != 0xFFFFFFFF
            refused += 1
        if kind == "fasta_header" and open(p, "rb").read(1) == b">":
            assert row["status"] == "badfirst"
        if r.returncode != 0:
            assert row["status"] != "ok", p
    assert refused > len(paths) // 2


def test_multi_line_golden_is_flagged(driver, work):
    p = str(work / "edge_p.fq")
    shutil.copyfile(os.path.join(GOLDEN, "s00_edge_k31", "p.fq"), p)
    row = run_driver(driver, 1 << 24, [p])[0]
    assert row["status"] == "flagged" and row["first_bad"] != 0xFFFFFFFF, row["line"]


@pytest.mark.parametrize("sanitize", [False, True])
def test_newline_bits_of_a_word_equal_a_byte_loop(work, sanitize):
    """nl_bits4 (hast_amd/csrc/nl_index.h), the step of the newline index that the framers of `classify` and of this ingest share:
    tests/native/test_nl_index.cpp holds it to a byte loop on every word over the neighbours of '\\n'"""
    out = os.path.join(str(work), "test_nl_index_san" if sanitize else "test_nl_index")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra"] + (["-fsanitize=address,undefined"] if sanitize else []) +
                   ["-o", out, os.path.join(sc.ROOT, "tests", "native", "test_nl_index.cpp")], check=True)
    r = subprocess.run([out], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and r.stdout.startswith(b"ok 65536 words") and r.stderr == b"", (r.stdout, r.stderr)
