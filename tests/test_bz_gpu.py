"""The per-member device inflate of blocked gzip (include/hast.h hast_gz_open_blocked, hast_amd/csrc/bz_kernels.hip) through the
C ABI, against zlib's bytes: every file of tests/bz_corpus.py at the default geometry, at batches of one to three members and at
batches of a few dozen, read in large, odd and tiny pieces; every damaged file delivers exactly the bytes of the members in front of
the bad one and then an error, never other data; what is no blocked gzip is refused at open; a stream closed with batches in flight."""
import os
import stat

import pytest

import hast_amd
from tests import bz_corpus as bc

pytestmark = pytest.mark.gpu

GEOMETRIES = ((0, 0), (70 << 10, 64 << 10), (300 << 10, 1 << 20))
HAST_ERR_IO, HAST_ERR_UNSUPPORTED = 8, 9


@pytest.fixture(scope="module")
def ctx():
    if not os.path.exists(hast_amd.lib_path()):
        hast_amd.build()
    with hast_amd.Context(21) as c:
        yield c


def n_members(f):
    at, n = 0, 0
    while True:
        ht = bc.walk_header(f, at)
        if ht is None:
            return n
        at += ht[1]
        n += 1


@pytest.mark.parametrize("name", sorted(bc.GOOD))
def test_good_files_give_zlibs_bytes(ctx, tmp_path, name):
    f, data = bc.GOOD[name]
    p = tmp_path / (name + ".gz")
    p.write_bytes(f)
    for batch_in, batch_out in GEOMETRIES:
        for piece in (1 << 22, 65537, 13):
            if piece == 13 and name not in bc.SMALL:
                continue
            with hast_amd.GzReader.blocked(ctx, str(p), batch_in, batch_out) as z:
                got = z.read_all(piece)
                st, bs = z.stats(), z.blocked_stats()
                assert z.units() == 1
            assert got == data, (name, batch_in, batch_out, piece, len(got), len(data))
            assert st["out_bytes"] == len(data) and st["compressed_bytes"] == len(f) and st["members"] == n_members(f), (name, st)
            assert bs["members"] == st["members"] and bs["unsupported_offset"] == 0
            if batch_out == 64 << 10 and len(data) > 140_000:
                assert bs["batches"] > 1, (name, bs)
            if batch_in == 300 << 10 and len(f) > 400_000:                 # (fastq_tiny_members: 487 KB of members)
                assert bs["batches"] > 1, (name, bs)


@pytest.mark.parametrize("name", sorted(bc.BAD))
def test_bad_files_deliver_the_members_in_front_and_then_an_error(ctx, tmp_path, name):
    f, head, kind, idx, reason = bc.BAD[name]
    p = tmp_path / (name + ".gz")
    p.write_bytes(f)
    for batch_in, batch_out in GEOMETRIES:
        for piece in (1 << 22, 65537, 999):
            got = b""
            with hast_amd.GzReader.blocked(ctx, str(p), batch_in, batch_out) as z:
                with pytest.raises(hast_amd.HastError) as ei:
                    for _ in range(100_000):
                        a = z.read(piece)
                        assert a.size > 0, "the stream ended as if it were complete"
                        got += a.tobytes()
                bs = z.blocked_stats()
            # exactly the members in front of the bad one: not a byte of it or behind it (for the too-far match in particular not the
            # previous member's bytes)
            assert got == head, (name, batch_in, batch_out, piece, len(got), len(head))
            if kind == "unsupported":
                assert ei.value.status == HAST_ERR_UNSUPPORTED and str(bc.unsupported_offset(name)) in str(ei.value), str(ei.value)
                assert bs["unsupported_offset"] == bc.unsupported_offset(name)
            else:
                assert ei.value.status == HAST_ERR_IO, str(ei.value)
                assert os.path.basename(str(p)) in str(ei.value)


def test_what_is_not_blocked_gzip_is_refused_at_open(ctx, tmp_path):
    from tests.test_inflate_cpu import member
    plain, empty, fifo = tmp_path / "plain.gz", tmp_path / "empty.gz", tmp_path / "fifo.gz"
    plain.write_bytes(member(b"ACGT\n" * 1000))
    empty.write_bytes(b"")
    os.mkfifo(fifo)
    assert stat.S_ISFIFO(os.stat(fifo).st_mode)
    for q in (plain, empty, fifo):
        with pytest.raises(hast_amd.HastError) as ei:
            hast_amd.GzReader.blocked(ctx, str(q))
        assert ei.value.status == HAST_ERR_UNSUPPORTED, (q, str(ei.value))
    with pytest.raises(hast_amd.HastError) as ei:
        hast_amd.GzReader.blocked(ctx, str(tmp_path / "missing.gz"))
    assert ei.value.status == HAST_ERR_IO
    # ... and the ordinary file still opens the ordinary way
    with hast_amd.GzReader(ctx, str(plain)) as z:
        assert z.read_all() == b"ACGT\n" * 1000
        with pytest.raises(hast_amd.HastError):
            z.blocked_stats()


def test_close_with_batches_in_flight_then_open_again(ctx, tmp_path):
    f, data = bc.GOOD["fastq_l6"]
    p = tmp_path / "f.gz"
    p.write_bytes(f)
    for batch_in, batch_out in ((70 << 10, 64 << 10), (0, 0)):
        z = hast_amd.GzReader.blocked(ctx, str(p), batch_in, batch_out)
        a = z.read(1000)
        assert a.tobytes() == data[:1000]
        z.close()                                                      # (the producer is ahead by up to three batches)
        with hast_amd.GzReader.blocked(ctx, str(p), batch_in, batch_out) as z2:
            assert z2.read_all(333_333) == data
    z = hast_amd.GzReader.blocked(ctx, str(p), 70 << 10, 64 << 10)
    z.close()                                                          # never read
