"""Host-only test of the DEVICE deflate encoder's per-piece code (hast_amd/csrc/dz_core.h), driven by tests/native/test_dz_core.cpp
with plain loops standing in for the wave of k_dz_piece: every output is one gzip member that zlib inflates to the input (CRC-32 and
ISIZE checked: wbits=31), that gz_core.h's decode_chunk reads back to the same bytes (checked in the driver: the project's decoder
against its encoder without zlib in between), whose Huffman codes are complete and within 15 / 7 bits, and that is no longer than
hast_dz_bound.  The corpus is where deflate encoders break: no distance code in use, a single symbol, lengths over 15, stored
fallback, matches of 258 at distance 1, the piece's borders.  Built with ASAN + UBSAN.  (tests/test_dz_gpu.py runs the same corpus
through the kernels; tests/test_dz_model_gpu.py holds the kernels to THIS model byte for byte, so what is asserted of the model
here -- the fuzz, the sizes around the laps of k_dz_scan, the size against zlib level 1 -- is asserted of the kernels too.)"""
import functools
import gzip
import math
import os
import random
import subprocess
import zlib

import numpy as np
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


def build_driver(directory, sanitize=True):
    """tests/native/test_dz_core.cpp compiled into directory: with ASAN + UBSAN, or (for inputs of megabytes) with -O2 alone"""
    exe = os.path.join(str(directory), "test_dz_core" if sanitize else "test_dz_core_o2")
    how = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.run(["g++"] + how + ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "test_dz_core.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("dzcore"))


@pytest.fixture(scope="module")
def fast_driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("dzcore_o2"), sanitize=False)


def compress(driver, tmp_path, data, literals_only=False):
    src, dst = tmp_path / "in.bin", tmp_path / "out.gz"
    src.write_bytes(data)
    r = subprocess.run([driver] + (["-H"] if literals_only else []) + [str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr[-400:]
    pieces, stored, size, limited = (int(x) for x in r.stdout.split())
    blob = dst.read_bytes()
    assert size == len(blob)
    return blob, pieces, stored, limited


def compress_with_sizes(driver, tmp_path, data, literals_only=False):
    """the driver's -v: (the member, the bytes each piece takes in it)"""
    src, dst = tmp_path / "in.bin", tmp_path / "out.gz"
    src.write_bytes(data)
    r = subprocess.run([driver, "-v"] + (["-H"] if literals_only else []) + [str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr[-400:]
    first, second = r.stdout.split(b"\n")[:2]
    pieces, _, size, _ = (int(x) for x in first.split())
    sizes = [int(x) for x in second.split()]
    blob = dst.read_bytes()
    assert size == len(blob) == 10 + sum(sizes) + 10 and len(sizes) == pieces == (len(data) + PIECE - 1) // PIECE
    return blob, sizes


# ---- inputs shared with tests/test_dz_model_gpu.py ------------------------------------------------------------------------------
COPY_DISTANCES = (1, 2, 3, 63, 64, 65, 4095, 4096, 16383, 16384, 16385)     # around a step of 64 positions, the table's 4096 entries, a piece
FUZZ_MAX = 70_000


def _some_length(rng, most):
    """1 .. most, short lengths as likely as long ones"""
    return min(most, int(math.exp(rng.uniform(0, math.log(most + 1)))))


def fuzz_input(rng):
    """0 .. 70 000 bytes put together from segments of random length: FASTQ records, bytes over 2, 4 or 20 symbols, incompressible
    bytes, a run of one byte (1 .. 70 000), a pattern of period 2 .. 300, a copy of what lies a chosen distance back"""
    edges = (0, 1, 2, 3, 4, 5, 63, 64, 65, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE, 4 * PIECE, 4 * PIECE + 3, FUZZ_MAX)
    target = rng.choice(edges) if rng.random() < 0.15 else rng.randint(0, FUZZ_MAX)
    out = bytearray()
    while len(out) < target:
        kind = rng.choice(("fastq", "alphabet", "noise", "run", "period", "copy", "copy"))
        if kind == "fastq":
            seg = fastq(rng, rng.randint(1, 30))
            seg = seg[:_some_length(rng, len(seg))]
        elif kind == "alphabet":
            symbols = bytes(rng.sample(range(256), rng.choice((2, 4, 20))))
            seg = bytes(rng.choices(symbols, k=_some_length(rng, 20_000)))
        elif kind == "noise":
            n = _some_length(rng, 20_000)
            seg = rng.getrandbits(8 * n).to_bytes(n, "little")
        elif kind == "run":
            seg = bytes([rng.getrandbits(8)]) * _some_length(rng, FUZZ_MAX)
        elif kind == "period":
            period = rng.randint(2, 300)
            pattern = bytes(rng.choices(b"ACGTN\n" if rng.random() < 0.5 else bytes(range(256)), k=period))
            n = _some_length(rng, 20_000)
            seg = (pattern * (n // period + 1))[:n]
        else:
            near = [d for d in COPY_DISTANCES if d <= len(out)]
            if not near:
                continue
            d = rng.choice(near)
            n = _some_length(rng, 3000)
            seg = (bytes(out[-d:]) * (n // d + 1))[:n]      # (as a match does it: longer than its distance, it repeats)
        out += seg
    return bytes(out[:target])


@functools.lru_cache(maxsize=None)
def fuzz_inputs():
    """the fuzz corpus: HAST_FUZZ_SEED (a fixed default), HAST_FUZZ_ITERS inputs (150 at least)"""
    rng = random.Random(int(os.environ.get("HAST_FUZZ_SEED", "20261017")))
    return [fuzz_input(rng) for _ in range(max(150, int(os.environ.get("HAST_FUZZ_ITERS", "160"))))]


def fastq_150(n_bytes, noisy, seed):
    """n_bytes of FASTQ with 150-bp records (headers as tests.test_inflate_cpu.fastq writes them), quality lines constant or over
    the alphabet FFFFF:F,F#; the last record is cut where n_bytes end"""
    rng = np.random.default_rng(seed)
    n = n_bytes // 320 + 1
    bases = rng.choice(np.frombuffer(b"ACGT", np.uint8), (n, 150))
    qual = rng.choice(np.frombuffer(b"FFFFF:F,F#", np.uint8), (n, 150)) if noisy else np.full((n, 150), ord("F"), np.uint8)
    data = b"".join(b"@V300R%09d#%d_%d_%d/1\n" % (i, i % 1536, i % 977, i % 3) + bases[i].tobytes() + b"\n+\n" + qual[i].tobytes() + b"\n" for i in range(n))
    assert len(data) >= n_bytes
    return data[:n_bytes]


def lap_sizes(piece=PIECE):
    """k_dz_scan places 256 pieces a lap: input sizes around the first and second lap's end, and one of 1227 pieces (five laps)"""
    return [255 * piece, 256 * piece - 1, 256 * piece, 256 * piece + 1, 257 * piece, 512 * piece + 7, 1227 * piece - 100]


@functools.lru_cache(maxsize=None)
def lap_content(kind):
    """the content the lap sizes are cut from: generated FASTQ (every piece coded), or the corpus's "mixed" tiled (95 000 bytes of
    FASTQ, noise, zeros, FASTQ: stored and coded pieces alternate, so the places of the pieces mix n + 5 and coded sizes)"""
    n = max(lap_sizes())
    if kind == "fastq":
        return fastq_150(n, True, 11)
    assert kind == "mixed_tiled"
    return (CORPUS["mixed"] * (n // len(CORPUS["mixed"]) + 1))[:n]


def zlib_level_1_in_pieces(data):
    """what zlib level 1 makes of the same pieces without history: raw deflate of every 16 KB, and 20 bytes of header and trailer"""
    total = 20
    for off in range(0, len(data), PIECE):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        total += len(c.compress(data[off:off + PIECE]) + c.flush())
    return total


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


# ---- the model on the inputs tests/test_dz_model_gpu.py compares the kernels on ---------------------------------------------------
def test_fuzz(driver, tmp_path):
    """the fuzz corpus through the driver under ASAN + UBSAN (its own checks: complete codes, matches that match, decode_chunk, the
    CRC by slices), zlib's round trip, the bound"""
    inputs = fuzz_inputs()
    assert len(inputs) >= 150 and max(len(d) for d in inputs) <= FUZZ_MAX
    for k, data in enumerate(inputs):
        blob, sizes = compress_with_sizes(driver, tmp_path, data)
        d = zlib.decompressobj(31)
        assert d.decompress(blob) == data and d.eof and d.unused_data == b"", (k, len(data))
        assert len(blob) <= bound(len(data)), (k, len(data))
        assert all(sz <= min(PIECE, len(data) - i * PIECE) + 5 for i, sz in enumerate(sizes)), (k, len(data))


@pytest.mark.parametrize("kind", ["fastq", "mixed_tiled"])
def test_sizes_around_the_laps_of_the_scan(fast_driver, tmp_path, kind):
    """the model at the sizes where k_dz_scan starts a new lap of 256 pieces (and the CRC terms of megabytes of bytes behind a piece:
    the driver checks the member's CRC-32 against the bytewise one, zlib checks it again)"""
    content = lap_content(kind)
    for n in lap_sizes():
        data = content[:n]
        blob, sizes = compress_with_sizes(fast_driver, tmp_path, data)
        d = zlib.decompressobj(31)
        assert d.decompress(blob) == data and d.eof and d.unused_data == b"", n
        assert len(blob) <= bound(n) and len(sizes) == (n + PIECE - 1) // PIECE
        full = sizes[:n // PIECE]                           # (a last piece of a byte is a stored block in any content)
        if kind == "fastq":
            assert all(sz < PIECE for sz in full), n
        else:
            assert any(sz == PIECE + 5 for sz in full) and any((a > PIECE) != (b > PIECE) for a, b in zip(full, full[1:])), n


@pytest.mark.parametrize("name", ["golden", "generated_constant_quality", "generated_noisy_quality"])
def test_no_larger_than_zlib_level_1_on_the_same_pieces(fast_driver, tmp_path, name):
    """the ratio, as a condition on the model (the kernels are held to the model's bytes): on FASTQ of a piece or more the member is
    no larger than zlib level 1 applied to the same 16-KB pieces one by one (the golden r1.fq: 76 360 against 79 486 bytes; 20 MB of
    generated FASTQ: 0.967 of it with constant quality lines, 0.979 with noisy ones).  Not for tiny runs: a member of 380 bytes pays
    a dynamic header."""
    data = {"golden": golden_fastq, "generated_constant_quality": lambda: fastq_150(2 << 20, False, 12),
            "generated_noisy_quality": lambda: fastq_150(2 << 20, True, 13)}[name]()
    assert len(data) >= PIECE
    blob = compress(fast_driver, tmp_path, data)[0]
    assert gzip.decompress(blob) == data
    print("%s: %d -> %d bytes, zlib level 1 in pieces %d" % (name, len(data), len(blob), zlib_level_1_in_pieces(data)))
    assert len(blob) <= zlib_level_1_in_pieces(data)


def test_member_layout(tmp_path):
    """dz::member_layout, the host's check of an encoder result before it copies members (tests/native/test_dz_members.cpp): back to
    back with 1 to 4 runs, empty runs in every position, a gap, an overlap, the last member ending at cap and one byte past it"""
    exe = str(tmp_path / "test_dz_members")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "native", "test_dz_members.cpp")], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr[-2000:].decode(errors="replace")
    assert r.stdout.startswith(b"ok cases=") and int(r.stdout.split(b"=")[1]) > 100, r.stdout
