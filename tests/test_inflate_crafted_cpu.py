"""Deflate streams zlib's encoder never writes (tests/gz_crafted_corpus.py: distances up to 32 768, 15-bit codes and 48-bit tokens,
blocks without distance codes, a lone distance code, 258 as 284 + 31, far matches behind stored and fixed blocks, code-length runs
over the alphabets' border; forged members whose matches reach in front of their own first byte; structures that are not deflate)
through every host inflate route: the serial decoder (fast_inflate.h), the threaded one (par_inflate.h), and the host half of the
device route (gz_core.h / gz_chain.h, lane by lane and the way k_gz_decode's wave does it) -- the bytes are zlib's, and what zlib
refuses is refused: an error, never other data.  The drivers are built with ASAN + UBSAN, as in the tests these fixtures come from.
(tests/test_gz_crafted_gpu.py runs the same files through the kernels.)"""
import re
import subprocess

import pytest

from tests.gz_crafted_corpus import LENIENT, MUST_FAIL, VALID
from tests.test_gz_core_cpu import driver_exe  # noqa: F401  (fixture: tests/native/test_gz_core.cpp)
from tests.test_inflate_cpu import PAR_SHAPES, driver  # noqa: F401  (fixture: tests/native/test_inflate.cpp)

SERIAL_SHAPES = ((1 << 20, 1 << 20), (97, 64), (1, 333))                # -p / -i
CORE_SHAPES = ((300, 5, 40), (64, 1000, 100), (700, 50, 1.0), (4096, 3, 12), (32768, 64, 12))      # -c / -s / -r


def run(cmd):
    r = subprocess.run([str(x) for x in cmd], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert b"AddressSanitizer" not in r.stderr and b"runtime error" not in r.stderr, (cmd, r.stderr[-2000:])
    return r


def routes(driver, driver_exe, path):
    """every (label, command line) a crafted file goes through"""
    for piece, inbuf in SERIAL_SHAPES:
        yield ("serial", piece, inbuf), [driver, "-p", piece, "-i", inbuf, path]
    for chunk, threads, piece in PAR_SHAPES:
        yield ("par", chunk, threads, piece), [driver, "-P", "-c", chunk, "-t", threads, "-p", piece, path]
    for wave in ((), ("-w",)):
        for chunk, seg, room in CORE_SHAPES:
            yield ("gz_core",) + wave + (chunk, seg, room), [driver_exe, *wave, "-c", chunk, "-s", seg, "-r", room, path]


@pytest.mark.parametrize("name", sorted(VALID))
def test_valid_streams_give_zlibs_bytes(driver, driver_exe, tmp_path, name):
    blob, want = VALID[name]
    p = tmp_path / (name + ".gz")
    p.write_bytes(blob)
    for label, cmd in routes(driver, driver_exe, p):
        r = run(cmd)
        assert r.returncode == 0, (name, label, r.stderr[-300:])
        assert r.stdout == want, (name, label, len(r.stdout), len(want))


def test_a_block_rolled_back_at_the_buffer_end_leaves_no_reach_behind(driver, tmp_path):
    """`zero_codes_are_a_far_match` through the threaded decoder with chunks far smaller than its 375-byte blocks: a block that
    straddles the end of the input buffer is decoded on into the zero padding -- where zeros are matches at distance 24 577 -- and
    rolled back; what those tokens "read" of the history must be rolled back with it, or the chunk is refused for a reach in front
    of its member (it lies in the member's first 24 KB) that the stream never made"""
    blob, want = VALID["zero_codes_are_a_far_match"]
    p = tmp_path / "zero_codes.gz"
    p.write_bytes(blob)
    for chunk, threads in ((64, 1), (64, 2), (64, 5), (100, 2), (100, 3), (200, 2), (300, 4)):
        r = run([driver, "-P", "-c", chunk, "-t", threads, "-p", 65536, p])
        assert r.returncode == 0, (chunk, threads, r.stderr[-300:])
        assert r.stdout == want, (chunk, threads, len(r.stdout), len(want))


def test_ladder15_reaches_the_second_level_tables_and_far_copies(driver_exe, tmp_path):
    """what the wave's steps on `ladder15` are made of (-w -S): steps that parse with the second-level tables (a code longer than 9 /
    6 bits at a step's start), rounds that copy from further back than the ring of recent symbols, long matches that do"""
    blob, want = VALID["ladder15"]
    p = tmp_path / "ladder15.gz"
    p.write_bytes(blob)
    r = run([driver_exe, "-w", "-S", "-c", 4096, str(p)])
    assert r.returncode == 0 and r.stdout == want
    m = re.search(rb"with second-level tables (\d+)\).* with_far_copy (\d+) .* long_far (\d+)", r.stderr)
    assert m, r.stderr[-300:]
    full, with_far, longs_far = (int(x) for x in m.groups())
    print("second-level steps %d, rounds with a far copy %d, long far matches %d" % (full, with_far, longs_far))
    assert full > 0 and with_far > 0 and longs_far > 0


def test_small_blocks_put_more_than_two_groups_through_the_chain(driver_exe, tmp_path):
    """`far_small_blocks` at 256-byte chunks: nearly every chunk holds a block start, and the chain accepts chunk after chunk -- more
    than two groups of 64 for the window kernels of the device route (the same count is asserted there)"""
    blob, want = VALID["far_small_blocks"]
    p = tmp_path / "small.gz"
    p.write_bytes(blob)
    for wave in ((), ("-w",)):
        r = run([driver_exe, *wave, "-S", "-c", 256, "-s", 5, "-r", 40, str(p)])
        assert r.returncode == 0 and r.stdout == want
        m = re.search(rb"chain accepted (\d+) chunks", r.stderr)
        assert m, r.stderr[-300:]
        print("accepted", int(m.group(1)))
        assert int(m.group(1)) >= 130


@pytest.mark.parametrize("name", sorted(MUST_FAIL))
def test_what_zlib_refuses_is_refused(driver, driver_exe, tmp_path, name):
    """an error on every route (the drivers exit with 3), no sanitizer report, and what was written before it is a prefix of the valid
    bytes in front of the damage -- the trailers of these files are right for what a lenient decoder would produce, so the CRC-32
    does not catch what the decoder lets through"""
    blob, prefix = MUST_FAIL[name]
    p = tmp_path / (name + ".gz")
    p.write_bytes(blob)
    accepted = []
    for label, cmd in routes(driver, driver_exe, p):
        r = run(cmd)
        if r.returncode == 0:
            accepted.append(label)
            continue
        assert r.returncode == 3, (name, label, r.returncode, r.stderr[-300:])
        assert prefix.startswith(r.stdout), (name, label, len(r.stdout), len(prefix))
    assert not accepted, (name, accepted)


@pytest.mark.parametrize("name", sorted(LENIENT))
def test_lenient_cases_give_an_error_or_the_simulated_bytes(driver, driver_exe, tmp_path, name):
    """incomplete codes that never miss: zlib refuses them, the bytes are well defined -- a route may do either, nothing else"""
    blob, want = LENIENT[name]
    p = tmp_path / (name + ".gz")
    p.write_bytes(blob)
    verdicts = {}
    for label, cmd in routes(driver, driver_exe, p):
        r = run(cmd)
        assert r.returncode in (0, 3), (name, label, r.returncode, r.stderr[-300:])
        if r.returncode == 0:
            assert r.stdout == want, (name, label)
        else:
            assert want.startswith(r.stdout), (name, label)
        verdicts.setdefault(label[0] + ("_wave" if "-w" in label else ""), set()).add(r.returncode)
    print(name, dict((k, sorted(v)) for k, v in verdicts.items()))
