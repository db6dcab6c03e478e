"""Host-only test of the BLOCKED framing of the device deflate encoder (hast_amd/csrc/dz_core.h: members of three pieces with a BC
header, CRC-32 and ISIZE each -- BGZF), driven by tests/native/test_dz_blocked.cpp, which restates k_dz_scan<true> and k_dz_gather
with plain loops and checks them against dz::blocked_run, bz::parse_header and bz::plan_batch (ASAN + UBSAN).  Here: zlib reads every
member back (CRC-32 and ISIZE checked: wbits=31), the members tile the input in slices of 49 152 bytes, the sizes against the bound
and against the ordinary member of the same pieces.  Sizes: around a piece, around a member, around the laps of the scan (256 pieces
a lap, and 256 is no multiple of 3: member 85 holds pieces 255, 256 and 257).  tests/test_dz_blocked_gpu.py holds the kernels to
this model byte for byte."""
import functools
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_dz_core_cpu import CORPUS, PIECE, bound, lap_content

MEMBER_INPUT = 3 * PIECE
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
SMALL_SIZES = (0, 1, 16383, 16384, 16385, 49151, 49152, 49153, 98304 + 7)
LAP_SIZES = tuple(p * PIECE + d for p in (255, 256, 257, 258) for d in (-1, 0, 1))
MANY_PIECES = 1227 * PIECE


def n_members(n):
    return (n + MEMBER_INPUT - 1) // MEMBER_INPUT


def bound_blocked(n):
    return n + 5 * ((n + PIECE - 1) // PIECE) + 28 * max(1, n_members(n))


def build_driver(directory, sanitize=True):
    """tests/native/test_dz_blocked.cpp compiled into directory: with ASAN + UBSAN, or (for inputs of megabytes) with -O2 alone"""
    exe = os.path.join(str(directory), "test_dz_blocked" if sanitize else "test_dz_blocked_o2")
    how = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.run(["g++"] + how + ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "test_dz_blocked.cpp")], check=True)
    return exe


def compress_blocked(driver, directory, data, emit_empty=True):
    """(the blocked bytes, pieces, stored pieces, members, the ordinary member's size) of the host model"""
    src, dst = os.path.join(str(directory), "in.bin"), os.path.join(str(directory), "out.bgzf")
    with open(src, "wb") as f:
        f.write(data)
    r = subprocess.run([driver] + ([] if emit_empty else ["-n"]) + [src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr[-600:].decode(errors="replace")
    pieces, stored, size, members, ordinary = (int(x) for x in r.stdout.split())
    blob = open(dst, "rb").read()
    assert size == len(blob)
    return blob, pieces, stored, members, ordinary


def walk_members(blob):
    """blob as a series of BGZF members: [(offset, member bytes, CRC-32, ISIZE)]; asserts the 18-byte header with the BC subfield,
    BSIZE, and that nothing but whole members is there"""
    out, at = [], 0
    while at < len(blob):
        h = blob[at:at + 18]
        assert len(h) == 18 and h[:4] == b"\x1f\x8b\x08\x04" and h[10:16] == b"\x06\x00BC\x02\x00", "byte %d: not a BGZF header: %s" % (at, h.hex())
        total = struct.unpack("<H", h[16:18])[0] + 1
        assert 28 <= total <= 65536 and at + total <= len(blob), (at, total)
        crc, isize = struct.unpack("<II", blob[at + total - 8:at + total])
        out.append((at, blob[at:at + total], crc, isize))
        at += total
    return out


def check_blocked(blob, data, emit_empty=True):
    """every member inflates (zlib checks CRC-32 and ISIZE) to its slice of 49 152 bytes; returns the number of members"""
    members = walk_members(blob)
    want = n_members(len(data)) if data else (1 if emit_empty else 0)
    assert len(members) == want, (len(members), want)
    at = 0
    for off, member, crc, isize in members:
        d = zlib.decompressobj(31)
        plain = d.decompress(member)
        assert d.eof and d.unused_data == b"", off
        assert plain == data[at:at + MEMBER_INPUT] and isize == len(plain) <= MEMBER_INPUT and crc == zlib.crc32(plain), off
        at += isize
    assert at == len(data)
    assert len(blob) <= bound_blocked(len(data))
    return len(members)


@functools.lru_cache(maxsize=None)
def noise(n):
    return np.random.default_rng(5).integers(0, 256, n, dtype=np.uint8).tobytes()


def sized_input(kind, n):
    if kind == "random":
        return noise(MANY_PIECES)[:n]
    content = lap_content(kind)                             # (100 bytes short of 1 227 pieces: it goes round)
    data = content[:n] + content[:max(0, n - len(content))]
    assert len(data) == n
    return data


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("dzblocked"))


@pytest.fixture(scope="module")
def fast_driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("dzblocked_o2"), sanitize=False)


def check_model(driver, tmp_path, data, what):
    blob, pieces, stored, members, ordinary = compress_blocked(driver, tmp_path, data)
    n = len(data)
    assert pieces == (n + PIECE - 1) // PIECE, what
    assert check_blocked(blob, data) == members, what
    assert ordinary <= bound(n), what
    if n:
        assert len(blob) == ordinary - 20 + 28 * n_members(n), what
    else:
        assert blob == EOF_BLOCK, what
    return blob, pieces, stored


def test_the_bound_is_the_issue_s():
    assert bound_blocked(0) == 28 and bound_blocked(1) == 1 + 5 + 28 and bound_blocked(MEMBER_INPUT) == MEMBER_INPUT + 15 + 28
    assert bound_blocked(MEMBER_INPUT + 1) == MEMBER_INPUT + 1 + 20 + 56
    assert 18 + 3 * (PIECE + 5) + 10 <= 65536 < 18 + 4 * (PIECE + 5) + 10


@pytest.mark.parametrize("name", sorted(CORPUS))
def test_the_corpus(driver, tmp_path, name):
    data = CORPUS[name]
    blob, pieces, stored = check_model(driver, tmp_path, data, name)
    if name == "random":
        assert stored == pieces and len(blob) == bound_blocked(len(data))


@pytest.mark.parametrize("kind", ["fastq", "mixed_tiled", "random"])
def test_sizes_around_a_piece_and_a_member(driver, tmp_path, kind):
    for n in SMALL_SIZES:
        blob, pieces, stored = check_model(driver, tmp_path, sized_input(kind, n), "%s, %d bytes" % (kind, n))
        if kind == "random":
            assert stored == pieces and len(blob) == bound_blocked(n), n


def test_an_empty_run_without_emit_empty_is_nothing(driver, tmp_path):
    blob, pieces, _, members, _ = compress_blocked(driver, tmp_path, b"", emit_empty=False)
    assert blob == b"" and pieces == 0 and members == 0
    blob, _, _, members, _ = compress_blocked(driver, tmp_path, b"A", emit_empty=False)
    assert members == 1 and check_blocked(blob, b"A", emit_empty=False) == 1


@pytest.mark.parametrize("kind", ["fastq", "mixed_tiled"])
def test_sizes_around_the_laps_of_the_scan(fast_driver, tmp_path, kind):
    """255, 256, 257 and 258 pieces, each a byte less and a byte more: member 85 (pieces 255, 256, 257) has one, two or three pieces
    and one, two or none of them in the second lap"""
    for n in LAP_SIZES:
        check_model(fast_driver, tmp_path, sized_input(kind, n), "%s, %d bytes" % (kind, n))


@pytest.mark.parametrize("kind", ["mixed_tiled", "random"])
def test_1227_pieces(fast_driver, tmp_path, kind):
    data = sized_input(kind, MANY_PIECES)
    blob, pieces, stored = check_model(fast_driver, tmp_path, data, kind)
    assert pieces == 1227 and len(walk_members(blob)) == 409
    if kind == "random":
        assert stored == pieces and len(blob) == bound_blocked(len(data))
