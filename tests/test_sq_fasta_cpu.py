"""The rules of the stage-00 device ingest of FASTA (hast_amd/csrc/sq_core.h, namespace sqfa), stepped on the host by
tests/native/test_sq_fasta.cpp the way hast_sq_feed_* steps them on the GPU (carry, open state, `last` at the end): at every block
size the stream is the host parser's (tests/native/test_seqstream.cpp, i.e. SeqParser) byte for byte, and the record and base totals
agree.  Run plain and as a stand-alone ASan + UBSan build of the program."""
import subprocess

import pytest

from tests import sq_fasta_corpus as fc


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """(name, paths, longest line, the parser's stream, records): written and parsed once"""
    d = tmp_path_factory.mktemp("sq_fasta_corpus")
    driver = fc.build_parser_driver(d)
    out = []
    for name, files, longest in fc.corpus():
        paths = fc.write_case(d, name, files)
        out.append((name, paths, longest, fc.parser_stream(driver, paths), fc.header_count(files)))
    return out


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("sq_fasta_model")
    return {False: fc.build_model(d), True: fc.build_model(d, sanitize=True)}


def test_issue_examples_are_the_parsers(cases):
    streams = {name: stream for name, _, _, stream, _ in cases}
    assert streams["issue_example"] == b"ACGT\n\n@r1+NNac\n"
    assert streams["only_header_nonl"] == b"\n"
    assert streams["issue_two_files"] == b"ACG\nTTT\n"


def test_corpus_covers_what_it_should():
    names = [c[0] for c in fc.corpus()]
    assert len(names) == len(set(names))
    for width in fc.WIDTHS:
        assert any(n.startswith("w%d_" % width) for n in names)
    for n in fc.COUNTS:
        assert any(x.startswith("n%d_" % n) for x in names)


@pytest.mark.parametrize("sanitize", (False, True), ids=("plain", "asan_ubsan"))
@pytest.mark.parametrize("block", fc.BLOCKS)
def test_model_stream_equals_the_parsers(cases, programs, block, sanitize):
    ran = 0
    for name, paths, longest, want, records in cases:
        if longest > block:
            continue
        res = subprocess.run([programs[sanitize], "-b", str(block), "-c"] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert res.returncode == 0, (name, block, res.stderr[-2000:])
        status, n_rec, n_bases, n_bytes, views = res.stdout.split()
        got = open(paths[0] + ".sqfa", "rb").read()
        assert status == b"ok" and got == want, (name, block)
        assert int(n_rec) == records and int(n_bases) == len(want) - want.count(b"\n"), (name, block)
        assert int(n_bytes) == sum(len(open(p, "rb").read()) for p in paths)
        ran += 1
    assert ran >= 50, (block, ran)


def test_a_line_longer_than_a_block_does_not_fit(cases, programs):
    name, paths, longest, _, _ = next(c for c in cases if c[0] == "w4097_b0")
    res = subprocess.run([programs[False], "-b", "700", "-c"] + paths, stdout=subprocess.PIPE, check=True)
    assert res.stdout.split()[0] == b"nofit"
