"""The thresholds that tests/rows_corpus.py derives BIG_N and TILE_SIZES from, read out of the sources of the output table's device step
as text, and the conditions the big cases have to meet for tests/test_rows_gpu.py to mean what it says.

test_rows_gpu.py runs a table just past ONE pass of the capped grids of rows_kernels.hip, past the size at which the library's radix sort
leaves its merge sort for Onesweep, and tables at the edge of a round of k_rows_scan.  If a tile, the cap, the scan's round or the
library's limit moves, those tables silently fall back under it and the second walk of the tile loops, the carries of the scan or the
Onesweep path are no longer run by anything.  This test then fails and says which constants to move."""
import os
import re
import shutil
import subprocess
from collections import Counter

import numpy as np
import pytest

from tests import rows_corpus as rc
from tests import rows_model as rm
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "hast_amd", "csrc")
MOVE = ("; tests/rows_corpus.py (TILE, GRID_CAP, SCAN_ROUND, SORT_MERGE_LIMIT -> BIG_N, TILE_SIZES) must follow it, or tests/test_rows_gpu.py no "
        "longer reaches the second walk of the tile loops, a second round of the scan or the sort past the library's merge sort")


def src(name):
    return open(os.path.join(CSRC, name)).read()


def constant(text, name):
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, text)
    assert m, "no constant %s" % name + MOVE
    return int(m.group(1))


def test_the_tile_and_the_grid_cap():
    assert constant(src("rows_device.h"), "kTile") == rc.TILE, "kTile of rows_device.h" + MOVE
    text = src("rows_kernels.hip")
    assert constant(text, "kGridCap") == rc.GRID_CAP, "kGridCap of rows_kernels.hip" + MOVE
    body = re.search(r"inline uint32_t grid_for\(size_t items\) \{(.*?)\}", text)
    assert body, "grid_for is no longer where it was" + MOVE
    # the cap is kGridCap and nothing else: no other number but the 1 of an empty grid, and the items are held against the cap
    assert re.findall(r"\b\d+\b", body.group(1)) == ["1"] and "items < kGridCap ?" in body.group(1) and body.group(1).count("kGridCap") == 2, body.group(1) + MOVE
    # every tile loop takes its grid from it, and strides by the grid
    grids = re.findall(r"hipLaunchKernelGGL\((k_rows_\w+), dim3\(([^;]*?)\), dim3\((\d+)\)", text)
    assert sorted(grids) == [("k_rows_gather", "grid_for((n + 255) / 256)", "256"), ("k_rows_key", "grid_for((n + 255) / 256)", "256"), ("k_rows_scan", "1", "256"),
                             ("k_rows_tile_sums", "grid_for(nt)", "256"), ("k_rows_write", "grid_for(n_tiles(n))", "256")], str(grids) + MOVE
    assert len(re.findall(r"for \(size_t t = blockIdx\.x; t < nt; t \+= gridDim\.x\)", text)) == 2, "the tile loops of k_rows_tile_sums and k_rows_write" + MOVE
    assert len(re.findall(r"for \(size_t \w = \(size_t\)blockIdx\.x \* 256 \+ threadIdx\.x; \w < n; \w \+= \(size_t\)gridDim\.x \* 256\)", text)) == 2, \
        "the id loops of k_rows_key and k_rows_gather" + MOVE


def test_the_scan_takes_256_tiles_a_round():
    text = src("rows_kernels.hip")
    assert re.findall(r"for \(size_t t0 = 0; t0 < nt; t0 \+= (\d+)\)", text) == [str(rc.SCAN_ROUND)], "k_rows_scan's round" + MOVE
    assert re.search(r"hipLaunchKernelGGL\(k_rows_scan, dim3\(1\), dim3\(%d\)," % rc.SCAN_ROUND, text), "k_rows_scan's launch" + MOVE


def test_the_sort_is_the_librarys_with_its_default_configuration():
    text = src("rows_sort.hip")
    calls = re.findall(r"rocprim::radix_sort_pairs(<[^(]*>)?\(", text)
    assert calls == [""], "sort_pass no longer calls rocprim::radix_sort_pairs without a configuration of its own: %s" % calls + MOVE
    assert "radix_sort_config" not in text and "merge_sort_limit" not in text, "rows_sort.hip names a configuration" + MOVE


def hip_compiler():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


def test_the_librarys_merge_sort_limit(tmp_path):
    """radix_sort_config<>::merge_sort_limit of the installed library, printed by tests/native/radix_sort_limit.cpp"""
    hipcc = hip_compiler()
    if hipcc is None:
        pytest.skip("no HIP compiler (HIPCC, /opt/rocm/bin/hipcc, hipcc on PATH): the library's headers cannot be compiled")
    exe = str(tmp_path / "radix_sort_limit")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-x", "hip", "-o", exe, os.path.join(ROOT, "tests", "native", "radix_sort_limit.cpp")], check=True)
    limit = int(subprocess.run([exe], check=True, stdout=subprocess.PIPE, timeout=60).stdout)
    assert limit == rc.SORT_MERGE_LIMIT, "the library's radix sort is a merge sort up to %d rows, the tests assume %d" % (limit, rc.SORT_MERGE_LIMIT) + MOVE


def test_sizes_follow_from_the_thresholds():
    n = rc.BIG_N
    assert n == 1_049_089 == (rc.GRID_CAP + 1) * rc.TILE + 1
    tiles = -(-n // rc.TILE)
    assert tiles == rc.GRID_CAP + 2 and n % rc.TILE == 1                          # workgroups 0 and 1 again; the last tile holds one row
    assert 2 * rc.GRID_CAP < -(-n // 256) <= 3 * rc.GRID_CAP                      # k_rows_key, k_rows_gather: three walks
    assert -(-tiles // rc.SCAN_ROUND) == 9 and tiles % rc.SCAN_ROUND == 2         # nine scan rounds, the last of two tiles
    assert n - rc.SORT_MERGE_LIMIT == 513
    assert rc.TILE_SIZES == (131_072, 131_073) and [-(-m // rc.TILE) for m in rc.TILE_SIZES] == [rc.SCAN_ROUND, rc.SCAN_ROUND + 1]
    assert max(rc.SIZES) < rc.GRID_CAP * 256                                      # (what cases() runs stays one walk of every loop: its ids as they were)


# ---- what the big cases hold -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    case = rc.big_case()
    return case, rm.build(*case[1:])


def test_the_big_case_is_what_it_was_made_to_be(big):
    (_, names, c0, c1, n0, n1, w0, w1), want = big
    n = len(names)
    assert n == rc.BIG_N and (n0, n1, w0, w1) == rc.PLAIN
    assert set(rc.special_names(True)) <= set(names) and sum(t.startswith(b"ABCDEFGH") and len(t) == 15 and t[8:].isdigit() for t in names) == 6000
    assert set(rc.special_counts(True)) <= set(zip(c0, c1))
    # the table and the flags
    assert 27_500_000 < len(want.table) < 29_500_000 and want.any_sep and want.past_int, len(want.table)
    # ids in no order of the texts: the order is far from the identity and from its reverse
    order = np.array(want.order)
    assert 0.4 * n < int((order[1:] > order[:-1]).sum()) < 0.6 * n
    # the lists of every scan round, the lists of every full tile
    cls = np.array(want.cls, dtype=np.uint8)[order]
    per_round = rc.SCAN_ROUND * rc.TILE
    rounds = [[int((cls[r:r + per_round] == l).sum()) for l in (1, 2, 3)] for r in range(0, n, per_round)]
    assert len(rounds) == 9 and min(min(r) for r in rounds) > 100, rounds
    assert all(min(r) > 30000 for r in rounds[:8]) and sum(rounds[8]) == rc.TILE + 1, rounds
    full = cls[:n // rc.TILE * rc.TILE].reshape(-1, rc.TILE)
    assert len(full) == rc.GRID_CAP + 1
    for l in (1, 2, 3):
        assert int(((full == l).sum(axis=1) == 0).sum()) == 0, "a full tile without a row of list %d" % l
    # rows that the second pass of the sort must leave in the order of the first: the same first key word
    sorted_names = [names[i] for i in want.order]
    groups = Counter(t[:8].ljust(8, b"\0") for t in sorted_names)
    shared = [v for v in groups.values() if v >= 2]
    assert len(shared) > 100_000 and sum(shared) > 300_000, (len(shared), sum(shared))
    at = [i for i, t in enumerate(sorted_names) if t[:8] == b"ABCDEFGH"]
    assert len(at) > 6000 and at[-1] - at[0] + 1 == len(at) and at[-1] // rc.TILE - at[0] // rc.TILE + 1 > 10, (len(at), at[0], at[-1])
    assert at[-1] // rc.TILE >= rc.GRID_CAP                                       # (it reaches into the tiles of the second walk)
    # exact ties and their neighbours, all three calls among them
    calls = {(a - n0 * (b // n1), b % n1): set() for a, b in ((n0, n1), (n0 + 1, n1), (n0, n1 + 1))}
    for t, a, b in zip(names[:20000], c0, c1):
        if a and b and a < 2 ** 31 and (a // n0 == b // n1) and ((a % n0, b % n1) in ((0, 0), (1, 0), (0, 1))) and t not in (b"0", b"0_0", b"0_0_0"):
            calls[(a % n0, b % n1)].add(rm.hap(t, a, b, n0, n1, w0, w1))
    assert calls == {(0, 0): {-1}, (1, 0): {0}, (0, 1): {1}}, calls


def test_the_layouts_are_the_records_and_counters_of_the_case(big):
    """text16 and counts4 without a loop over the rows: the same arrays as a plain restatement, row by row, on a case with every length"""
    _, names, c0, c1 = rc.make_case("n700", 700, 6, rc.WEIGHTED, big=True, sep=True)[:4]
    text, counts = rc.text16(names), rc.counts4(c0, c1)
    assert text.shape == (700, 16) and text.dtype == np.uint8 and counts.shape == (700, 4) and counts.dtype == np.uint64
    for i, (t, x, y) in enumerate(zip(names, c0, c1)):
        assert text[i].tobytes() == bytes([len(t)]) + t + b"\0" * (15 - len(t)), i
        assert [int(v) for v in counts[i]] == [x, y, (x * 7 + y) % 1000, 0], i
    assert rc.text16([]).shape == (0, 16) and rc.counts4([], []).shape == (0, 4)
    big_text = rc.text16(big[0][1])
    assert big_text.shape == (rc.BIG_N, 16) and set(big_text[:, 0].tolist()) == set(range(16))


@pytest.mark.parametrize("n", rc.TILE_SIZES)
def test_the_tile_cases_hold_whole_tiles_of_every_list(n):
    _, names, c0, c1, n0, n1, w0, w1 = rc.tile_case(n)
    want = rm.build(names, c0, c1, n0, n1, w0, w1)
    assert len(names) == n and all(len(t) == 15 for t in names[:1000]) and (n0, w0) == (n1, w1)
    assert [int(names[i]) for i in want.order] == list(range(n))                  # the sorted rank is the number itself
    assert all(len(str(v)) == 20 for v in set(c0) | set(c1))
    cls = np.array(want.cls, dtype=np.uint8)[np.array(want.order)]
    full = cls[:n // rc.TILE * rc.TILE].reshape(-1, rc.TILE)
    pure = {l: int((full == l).all(axis=1).sum()) for l in (1, 2, 3)}
    assert min(pure.values()) >= rc.SCAN_ROUND // 4, pure                         # a quarter of the tiles each, and as many mixed
    mixed = [t for t in range(len(full)) if len(set(full[t].tolist())) == 3]
    assert len(mixed) == rc.SCAN_ROUND // 4 and all((full[t] == 1 + (np.arange(t * rc.TILE, (t + 1) * rc.TILE) % 3)).all() for t in mixed)
    for t in range(len(full)):
        assert rc.tile_kind(t) == ("mixed" if t in mixed else "all_list%d" % full[t][0]), t
    n3 = int((cls == 3).sum())
    assert len(want.table) == 61 * n3 + 60 * (n - n3) and [len(x) for x in want.lists] == [16 * int((cls == l).sum()) for l in (1, 2, 3)]
    if n % rc.TILE == 1:                                                          # the second scan round: one tile of one row, on list 3
        assert cls[-1] == 3 and want.table[-61:-46] == b"%015d" % (n - 1)
    assert not want.any_sep and want.past_int
