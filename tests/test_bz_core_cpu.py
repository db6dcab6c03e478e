"""Host-only test of the blocked-gzip rules the device stream runs on (hast_amd/csrc/bz_core.h): every file of tests/bz_corpus.py is
walked and planned at batch limits from one member up, piece by piece, every planned member is decoded by gz_core.h's lane decoder
and held to ISIZE and CRC-32 with the helpers the check kernel uses (tests/native/test_bz_core.cpp, built with ASAN + UBSAN).  Python's
zlib gives the verdict the corpus expects, and the host reader (bgzf_reader.h), which now takes its header rule from bz_core.h,
still reads the files as before."""
import os
import re
import struct
import subprocess
import zlib

import pytest

from tests import bz_corpus as bc
from tests.conftest import ROOT

SAN = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
# (batch_in, batch_out, piece): limits of one member; a few; the device stream's small test geometry read in odd pieces; everything at once
GEOMETRIES = [(1, 1, 1 << 16), (70 << 10, 64 << 10, 70 << 10), (300 << 10, 1 << 20, 33_333), (8 << 20, 64 << 20, 8 << 20)]


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("bz")
    core, inflate = d / "test_bz_core", d / "test_inflate"
    subprocess.run(SAN + ["-o", str(core), os.path.join(ROOT, "tests", "native", "test_bz_core.cpp")], check=True)
    subprocess.run(SAN + ["-o", str(inflate), os.path.join(ROOT, "tests", "native", "test_inflate.cpp"), "-lz", "-pthread"], check=True)
    return str(core), str(inflate)


def run_core(exe, path, geom):
    r = subprocess.run([exe, str(path)] + [str(v) for v in geom], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr[-500:]
    return r.stdout, r.stderr.decode().strip().splitlines()[-1]


def test_the_corpus_is_what_it_says():
    """Python's zlib, member by member, agrees with the verdict the corpus states for every file"""
    for name, (f, data) in bc.GOOD.items():
        assert bc.reference(f) == (data, None), name
    for name, (f, head, kind, idx, reason) in bc.BAD.items():
        got, verdict = bc.reference(f)
        assert got == head and verdict is not None and verdict[0] == idx, (name, verdict)
        assert reason == "any" or verdict[1] == reason, (name, verdict)
        assert (kind == "unsupported") == (verdict[1] == "not_bgzf")
    # the forged member: a decoder that copied out of the previous member's tail would find trailer and size right
    f, head, _, idx, _ = bc.BAD["too_far"]
    at = 0
    for _ in range(idx):
        at += bc.walk_header(f, at)[1]
    hdr, total = bc.walk_header(f, at)
    crc, isize = struct.unpack("<II", f[at + total - 8:at + total])
    forged = zlib.decompressobj(-15, zdict=head[-32768:]).decompress(f[at + hdr:at + total - 8])
    assert len(forged) == isize and zlib.crc32(forged) == crc and forged[5:15] == head[-10:]


@pytest.mark.parametrize("name", sorted(bc.GOOD))
def test_good_files_plan_and_decode_to_zlibs_bytes(drivers, tmp_path, name):
    f, data = bc.GOOD[name]
    p = tmp_path / "f.gz"
    p.write_bytes(f)
    for geom in GEOMETRIES:
        out, verdict = run_core(drivers[0], p, geom)
        assert verdict.startswith("verdict ok"), (name, geom, verdict)
        assert out == data, (name, geom)
        m = re.match(r"verdict ok members=(\d+) batches=(\d+) carried=(\d+)", verdict)
        if geom[0] == 1:
            assert int(m.group(2)) >= len(data) // 65536                # at most 64 KB of output a batch
    out, verdict = run_core(drivers[0], p, (70 << 10, 64 << 10, 1000))
    assert out == data
    assert int(verdict.rsplit("=", 1)[1]) > 0 or len(f) < 3000         # pieces of 1000 bytes: members are carried


@pytest.mark.parametrize("name", sorted(bc.BAD))
def test_bad_files_are_refused_at_the_expected_member(drivers, tmp_path, name):
    f, head, kind, idx, reason = bc.BAD[name]
    want = bc.reference(f)[1][1] if reason == "any" else reason
    p = tmp_path / "f.gz"
    p.write_bytes(f)
    for geom in GEOMETRIES:
        out, verdict = run_core(drivers[0], p, geom)
        m = re.match(r"verdict bad member=(\d+) reason=(\w+) offset=(\d+)", verdict)
        assert m, (name, geom, verdict)
        assert out == head and int(m.group(1)) == idx, (name, geom, verdict)
        assert m.group(2) == want, (name, geom, verdict)
        if kind == "unsupported":
            assert int(m.group(3)) == bc.unsupported_offset(name)


def test_a_file_that_does_not_start_with_a_blocked_member(drivers, tmp_path):
    from tests.test_inflate_cpu import member
    for blob in (member(b"ACGT" * 100), b"plain text\n" * 10):
        p = tmp_path / "x.gz"
        p.write_bytes(blob)
        assert run_core(drivers[0], p, GEOMETRIES[1])[1] == "verdict unsupported_at_open"


def test_host_reader_behaves_as_before(drivers, tmp_path):
    """bgzf_reader.h calls bz_core.h's header rule: same bytes as zlib on the good files and on the file with an ordinary member in
    mid-file (the serial decoder takes over); a BC subfield behind another one is still not seen by its 18-byte probe"""
    files = dict(bc.GOOD)
    mixed = bc.BAD["plain_gzip_member"][0]
    files["plain_gzip_member"] = (mixed, None)
    for name, (f, data) in sorted(files.items()):
        p = tmp_path / "f.gz"
        p.write_bytes(f)
        if data is None:                                               # (zlib reads the mixed file as ordinary multi-member gzip)
            want = subprocess.run([drivers[1], "-z", str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            assert want.returncode == 0
            data = want.stdout
        for piece, threads in ((1 << 22, 4), (70_000, 2)):
            got = subprocess.run([drivers[1], "-b", "-p", str(piece), "-t", str(threads), str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            if name == "other_subfield_first":
                assert got.returncode == 4
                continue
            assert got.returncode == 0, (name, got.stderr[-300:])
            assert got.stdout == data, name                            # (the corpus' bytes are zlib's: test_the_corpus_is_what_it_says)
