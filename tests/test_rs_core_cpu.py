"""Host-only test of the rules of stage 03's device ingest (hast_amd/csrc/rs_core.h, stepped by the model of rs_host.h in
tests/native/test_rs_core.cpp the way `classify_read --ingest device` feeds a file): at every block size the framed records are those
of the reference's two getline loops (tests/rs_corpus.py restates them), byte for byte, and no file that fits is refused."""
import subprocess

import pytest

from tests import rs_corpus as rc

BLOCKS = (64, 100, 700, 4096, 65536)
FMT = {rc.FASTA: "fasta", rc.FASTQ: "fastq"}


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("rs_core")


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def driver(request, work):
    return rc.build_native(work, sanitize=request.param == "asan_ubsan")


@pytest.fixture(scope="module")
def corpus(work):
    """the inputs as files, with what the reference's reader makes of each and the most bytes a feed has to carry"""
    out = []
    for name, fmt, data in rc.corpus(rc.make_keys(3, 21)):
        p = work / name
        p.write_bytes(data)
        out.append((name, fmt, str(p), data, rc.read_file(fmt, data), rc.carry_bound(fmt, data)))
    return out


def run_driver(driver, fmt, block, paths):
    r = subprocess.run([driver, "-f", FMT[fmt], "-b", str(block)] + list(paths), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"runtime error" not in r.stderr and b"Sanitizer" not in r.stderr, r.stderr.decode()[-2000:]
    rows = []
    for line, p in zip(r.stdout.decode().splitlines(), paths):
        f = line.split(" : ")[0].split()
        rows.append(dict(status=f[0], records=int(f[1]), bases=int(f[2]), bytes=int(f[3]), views=int(f[4]), rows=open(p + ".rs", "rb").read(), line=line))
    assert len(rows) == len(paths)
    return rows


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("fmt", (rc.FASTA, rc.FASTQ))
def test_records_are_the_reference_readers(driver, corpus, fmt, block):
    use = [c for c in corpus if c[1] == fmt and c[5] <= block]             # nothing to carry exceeds the block
    assert len(use) >= (5 if block < 700 else 15) and any(len(c[3]) > 2 * block or block == 65536 for c in use)
    rows = run_driver(driver, fmt, block, [c[2] for c in use])
    for (name, _, _, data, want, _), row in zip(use, rows):
        if want == rc.ERR:
            assert row["status"] == "format_error" and row["rows"] == b"", (name, block, row["line"])
            continue
        assert row["status"] == "ok", (name, block, row["line"])          # never refused: the generator's condition
        assert row["rows"] == rc.rows_of(want), (name, block)
        assert row["records"] == len(want) and row["bases"] == sum(len(s) for _, s in want) and row["bytes"] == len(data), (name, row["line"])
        assert row["views"] == -(-len(data) // block) + 1, (name, row["line"])       # every block, then the empty last one


def test_the_corpus_holds_every_case(corpus):
    names = {c[0] for c in corpus}
    for w in rc.WIDTHS:
        assert "fa_w%d" % w in names and "fq_l%d" % w in names
    for n in rc.COUNTS:
        fa = next(c for c in corpus if c[0] == "fa_n%d" % n)
        fq = next(c for c in corpus if c[0] == "fq_n%d" % n)
        assert len(fa[4]) == n and len(fq[4]) == n
    by = {c[0]: c for c in corpus}
    assert b"\r\n" in by["fa_crlf"][3] and all(n.endswith(b"\r") for n, _ in by["fa_crlf"][4]) and any(b"\r" in s for _, s in by["fa_crlf"][4])
    assert b"\n\n" in by["fa_blank"][3] and by["fa_junk_only"][4] == [] and by["empty_fa"][4] == [] and by["empty_fq"][4] == []
    assert by["fa_junk"][4][0][0].startswith(b"r0 ") and (b"lonely", b"") in by["fa_header_only"][4] and (b"", b"") in by["fa_bare"][4]
    assert by["fa_header_only"][4][-1] == (b"at the end", b"")
    assert by["fa_unterminated_seq"][4][-1] == (b"last", b"ACGTACGTACGTACGTACGTACGT") and by["fa_one_unterminated"][4] == []
    assert len(by["fa_unterminated_header"][4]) == 60
    n0 = len(by["fq_tail1_nonl"][4])
    assert n0 == 30 and len(by["fq_tail1_nl"][4]) == 31 and by["fq_tail1_nl"][4][-1] == (b"tail x", b"")
    for lines in (2, 3):
        for e in ("nl", "nonl"):
            got = by["fq_tail%d_%s" % (lines, e)][4]
            assert len(got) == 31 and got[-1][0] == b"tail x" and len(got[-1][1]) == 45
    assert by["fq_empty_header"][4][0] == (b"", b"ACGT") and by["fq_empty_header"][4][-1] == (b"", b"")
    errs = [c[0] for c in corpus if c[4] == rc.ERR]
    assert len(errs) == 10 and all("err" in n for n in errs)


@pytest.mark.parametrize("fmt", (rc.FASTA, rc.FASTQ))
def test_a_record_larger_than_the_block_is_too_long(driver, work, fmt):
    import random
    rng = random.Random(5)
    keys = rc.make_keys(3, 21)
    recs = rc.records(rng, 20, (100,), keys) + [(b"long one", rc.seq_with_plants(rng, 6000, keys))] + rc.records(rng, 5, (100,), keys)
    data = rc.fasta_text(rng, recs, 60) if fmt == rc.FASTA else rc.fastq_text(recs)
    p = work / ("too_long_%d" % fmt)
    p.write_bytes(data)
    assert rc.carry_bound(fmt, data) > 2 * 2048                 # no view of two blocks holds the record: wherever the views end
    small, big = run_driver(driver, fmt, 2048, [str(p)])[0], run_driver(driver, fmt, 16384, [str(p)])[0]
    assert small["status"] == "too_long" and small["rows"] == b"", small["line"]
    assert big["status"] == "ok" and big["rows"] == rc.rows_of(rc.read_file(fmt, data))
