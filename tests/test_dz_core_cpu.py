"""Host-only test of the DEVICE deflate encoder's per-piece code (hast_amd/csrc/dz_core.h), driven by tests/native/test_dz_core.cpp
with plain loops standing in for the wave of k_dz_piece: every output is one gzip member that zlib inflates to the input (CRC-32 and
ISIZE checked: wbits=31), that gz_core.h's decode_chunk reads back to the same bytes (checked in the driver: the project's decoder
against its encoder without zlib in between), whose Huffman codes are complete and within 15 / 7 bits, and that is no longer than
hast_dz_bound.  The corpus is where deflate encoders break: no distance code in use, a single symbol, lengths over 15, stored
fallback, matches of 258 at distance 1, the piece's borders.  Built with ASAN + UBSAN.  (tests/test_dz_gpu.py runs the same corpus
through the kernels.)"""
import gzip
import os
import random
import subprocess
import zlib

import pytest

from tests.conftest import ROOT
from tests.test_inflate_cpu import fastq

PIECE = 16384


def golden_fastq():
    return gzip.open(os.path.join(ROOT, "tests", "golden", "rand_k21", "r1.fq.gz")).read()


def skewed(rng, n_symbols=18):
    """bytes with the counts 1, 2, 3, 5, 8, ... (with the end-of-block code's 1 in front: Fibonacci's numbers), shuffled, 10 944
    bytes in all (one piece): the unlimited Huffman code of such a histogram is as deep as it has symbols.  That is the histogram
    of the block's SYMBOLS only when the encoder codes literals alone -- a match search takes the frequent bytes out of it."""
    a, b, out = 1, 2, bytearray()
    for s in range(n_symbols):
        out += bytes([65 + s]) * a
        a, b = b, a + b
    out = list(out)
    rng.shuffle(out)
    return bytes(out)


def dz_corpus():
    rng = random.Random(21)
    noise = bytes(rng.getrandbits(8) for _ in range(32768))
    fq = fastq(rng, 1500)
    cases = {
        "fastq_generated": fq,
        "fastq_golden": golden_fastq(),
        "empty": b"",
        "one_byte": b"A",
        "zeros": bytes(100_000),
        "all_byte_values": bytes(range(256)),
        "all_byte_values_thrice": bytes(range(256)) * 3,
        "one_value": b"G" * 5000,
        "one_value_short": b"G" * 3,
        "literals_only": bytes(rng.choice(b"ACGT") for _ in range(3 * PIECE + 100)),
        "random": bytes(rng.getrandbits(8) for _ in range(50_000)),
        "distance_32768": noise + noise[:3000],
        "skewed": skewed(rng),
        "piece_minus_1": fq[:PIECE - 1],
        "piece": fq[:PIECE],
        "piece_plus_1": fq[:PIECE + 1],
        "three_pieces_and_7": fq[:3 * PIECE + 7],
        "mixed": fq[:20_000] + noise[:20_000] + bytes(30_000) + fq[20_000:45_000],
    }
    return cases


CORPUS = dz_corpus()


def bound(n):
    return 10 + n + 5 * ((n + PIECE - 1) // PIECE) + 10


def huffman_only(data):
    c = zlib.compressobj(6, zlib.DEFLATED, 31, 9, zlib.Z_HUFFMAN_ONLY)
    return c.compress(data) + c.flush()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("dzcore") / "test_dz_core"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(exe), os.path.join(ROOT, "tests", "native", "test_dz_core.cpp")], check=True)
    return str(exe)


def compress(driver, tmp_path, data, literals_only=False):
    src, dst = tmp_path / "in.bin", tmp_path / "out.gz"
    src.write_bytes(data)
    r = subprocess.run([driver] + (["-H"] if literals_only else []) + [str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr[-400:]
    pieces, stored, size, limited = (int(x) for x in r.stdout.split())
    blob = dst.read_bytes()
    assert size == len(blob)
    return blob, pieces, stored, limited


def test_the_piece_size_is_the_one_the_tests_assume(driver):
    assert int(subprocess.run([driver, "-P"], stdout=subprocess.PIPE, check=True).stdout) == PIECE


@pytest.mark.parametrize("name", sorted(CORPUS))
def test_zlib_and_the_projects_decoder_read_it_back(driver, tmp_path, name):
    data = CORPUS[name]
    blob, pieces, stored, _ = compress(driver, tmp_path, data)
    d = zlib.decompressobj(31)
    assert d.decompress(blob) == data and d.eof and d.unused_data == b""
    assert len(blob) <= bound(len(data))
    assert pieces == (len(data) + PIECE - 1) // PIECE
    assert blob[:4] == b"\x1f\x8b\x08\x00"
    if name == "random":
        assert stored == pieces                          # (the fallback: random bytes do not get longer than stored blocks)
    if name in ("zeros", "one_value", "fastq_golden", "literals_only"):
        assert stored == 0


def test_length_and_distance_symbols_are_what_the_decoder_adds_up(driver):
    """every length 3 .. 258 and every distance 1 .. 32768 -> code, extra bits, extra value against gz_core.h's tables: the corpus
    cannot reach distances past 16 383 (pieces of 16 KB share no history; "distance_32768" is a round trip across pieces), so the
    upper distance codes are checked here"""
    r = subprocess.run([driver, "-s"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and r.stdout == b"ok\n", r.stderr[-300:]


def test_same_input_same_bytes(driver, tmp_path):
    a = compress(driver, tmp_path, CORPUS["fastq_generated"])[0]
    b = compress(driver, tmp_path, CORPUS["fastq_generated"])[0]
    assert a == b


def test_runs_become_matches_of_258_at_distance_1(driver, tmp_path):
    blob = compress(driver, tmp_path, CORPUS["zeros"])[0]
    assert len(blob) < len(CORPUS["zeros"]) // 100


def test_lengths_over_15_are_limited(driver, tmp_path):
    """the skewed input coded without matches has a literal/length tree 18 deep: the driver says how many pieces it had to limit (and
    checks every code of every piece for completeness); -k N does the same for a bare histogram of N symbols"""
    data = CORPUS["skewed"]
    blob, _, stored, limited = compress(driver, tmp_path, data, literals_only=True)
    assert limited == 1 and stored == 0
    assert gzip.decompress(blob) == data
    for n, want in ((2, 1), (16, 15), (17, 15), (30, 15), (286, 15)):
        r = subprocess.run([driver, "-k", str(n)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr[-300:]
        assert int(r.stdout) == want, n


def test_it_compresses(driver, tmp_path):
    """the size condition of tests/test_dz_gpu.py on the host model: matches are found and coded, so a FASTQ with constant quality
    lines gets smaller than zlib's Huffman-only coding of the same bytes (computed here)"""
    data = CORPUS["fastq_golden"]
    assert len(data) == 347531
    blob = compress(driver, tmp_path, data)[0]
    assert len(blob) < len(huffman_only(data))
