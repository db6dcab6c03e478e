"""The grid caps and tile sizes that tests/past_grid_corpus.py derives its sizes from, read out of the kernel sources as text.

tests/test_past_one_grid_gpu.py feeds every framing, routing, binning and conversion kernel a view just past ONE pass of its capped
grid.  If a cap or a tile is retuned, those views silently fall back under it and the second pass of the tile loops is no longer run by
anything.  This test then fails and says which sizes to move."""
import os
import re

from tests import past_grid_corpus as pg
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "hast_amd", "csrc")
MOVE = ("; tests/past_grid_corpus.py (GRID_CAP, NAME_GRID_CAP, TILE, COPY_TILE, NL_TILE, SCAN_THREADS -> N2, N1, EDGES, B) must follow it, "
        "and with it the block sizes of tests/test_past_one_grid_gpu.py, or those tests no longer reach the second pass of the tile loops")


def src(name):
    return open(os.path.join(CSRC, name)).read()


def constant(text, name):
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, text)
    assert m, "no constant %s" % name
    return int(m.group(1))


def test_capped_grid_caps_at_2048():
    body = re.search(r"inline uint32_t capped_grid\(size_t items, uint32_t per, uint32_t cap = (\d+)\) \{(.*?)\n\}", src("nl_index.h"), re.S)
    assert body, "capped_grid is no longer where it was" + MOVE
    assert int(body.group(1)) == pg.GRID_CAP, "capped_grid caps at %s by default, the tests assume %d" % (body.group(1), pg.GRID_CAP) + MOVE
    # the cap is the parameter and nothing else: no other number in the body, and the tiles are held against `cap`
    assert not re.findall(r"\b(\d{3,})\b", body.group(2)) and re.search(r"t < cap \? t : cap", body.group(2)), "capped_grid's body" + MOVE
    # every loop the big views are meant for takes its grid from it
    for name, n in (("rs_kernels.hip", 2), ("sq_kernels.hip", 1), ("sq_fasta_kernels.hip", 1), ("tx_kernels.hip", 1)):
        calls = re.findall(r"capped_grid\(([^;]*?)\)[,;]", src(name))
        assert len(calls) >= n, name + MOVE
        assert all(re.fullmatch(r"[^,]+, k\w+Tile", c) for c in calls), "%s passes a cap of its own: %s" % (name, calls) + MOVE


def test_tile_constants():
    want = {"rs_device.h": [("kRsTile", pg.TILE)], "sq_device.h": [("kSqRecTile", pg.TILE), ("kSqFaTile", pg.TILE)], "tx_device.h": [("kTxTile", pg.TILE)],
            "fq_device.h": [("kRouteTile", pg.TILE)], "span_copy.h": [("kSpanCopyTile", pg.COPY_TILE)], "nl_index.h": [("kNlTile", pg.NL_TILE)]}
    for name, constants in want.items():
        text = src(name)
        for c, v in constants:
            assert constant(text, c) == v, "%s is %d in %s, the tests assume %d" % (c, constant(text, c), name, v) + MOVE


def test_fixed_grids_of_the_fq_kernels():
    text = src("fq_kernels.hip")
    for kernel, cap in ((r"k_route_class<true>", pg.NAME_GRID_CAP), (r"k_route_class<false>", pg.NAME_GRID_CAP), (r"k_route_copy", pg.GRID_CAP),
                        (r"k_fq_records", pg.GRID_CAP), (r"k_fq_records_striped", pg.GRID_CAP)):
        grids = re.findall(r"hipLaunchKernelGGL\(%s,\s*dim3\((\d+)\)" % re.escape(kernel), text)
        assert grids and all(int(g) == cap for g in grids), "%s is launched with %s workgroups, the tests assume %d" % (kernel, grids, cap) + MOVE


def test_name_insert_and_tally_launches_cap_at_1024():
    text = src("fq_kernels.hip")
    for kernel, launches in (("k_fq_name_claim", 1), ("k_fq_name", 1), ("k_names_insert", 1), ("k_tally_add", 1)):
        grids = re.findall(r"hipLaunchKernelGGL\(%s,\s*dim3\(capped_grid\(\w+, (\d+), (\d+)\)\), dim3\((\d+)\)" % kernel, text)
        assert len(grids) == launches, (kernel, grids, MOVE)
        assert all(int(per) == int(block) == pg.TILE and int(cap) == pg.NAME_GRID_CAP for per, cap, block in grids), \
            "%s: %s, the tests assume a cap of %d" % (kernel, grids, pg.NAME_GRID_CAP) + MOVE
    m = re.search(r"const dim3 grid\(capped_grid\(most, (\d+), (\d+)\)\);", text)
    assert m and int(m.group(1)) == pg.TILE and int(m.group(2)) == pg.NAME_GRID_CAP, "k_fq_field2's grid" + MOVE
    for kernel in ("k_fq_field2<true>", "k_fq_field2<false>"):
        assert re.search(r"hipLaunchKernelGGL\(%s, grid, dim3\(256\)" % re.escape(kernel), text), kernel + MOVE


def test_the_block_scan_takes_ceil_n_over_1024_a_thread():
    text = src("scan_device.h")
    m = re.search(r"block_exclusive_scan_1024\(uint32_t \*v, uint32_t n, uint32_t \*s_part\) \{\s*const uint32_t per = \(n \+ (\d+)\) / (\d+),", text)
    assert m and int(m.group(1)) + 1 == int(m.group(2)) == pg.SCAN_THREADS, "block_exclusive_scan_1024" + MOVE
    assert len(re.findall(r"__launch_bounds__\(1024\)", src("rs_kernels.hip"))) >= 4


def test_sizes_follow_from_the_caps():
    assert pg.N2 == 524_609 and pg.N1 == 262_465 and pg.EDGES == (524_288, 524_289) and pg.B == 8_388_608
    for n, cap in ((pg.N2, pg.GRID_CAP), (pg.N1, pg.NAME_GRID_CAP)):
        t = -(-n // pg.TILE)
        assert t == cap + 2 and n % pg.TILE == 65 and 0 < n % 64 < 64          # workgroups 0 and 1 again; the last tile ends inside a wave
    assert -(-pg.EDGES[0] // pg.TILE) == pg.GRID_CAP and -(-pg.EDGES[1] // pg.TILE) == pg.GRID_CAP + 1
    assert -(-pg.N2 // pg.TILE) > 2 * pg.NAME_GRID_CAP                          # three passes of the kernels capped at 1024


def test_scan_runs_cover_every_tile_once():
    """the index arithmetic of block_exclusive_scan_1024, restated in past_grid_corpus.scan_runs: at n = 2050 every thread up to 682 takes
    three tiles, thread 683 one, the rest none"""
    for n in (0, 1, 1023, 1024, 1025, 2047, 2048, 2049, 2050, 3 * 2050, 4097, 65536 + 5):
        runs = pg.scan_runs(n)
        covered = [i for lo, hi in runs for i in range(lo, hi)]
        assert covered == list(range(n)), n
        per = -(-n // pg.SCAN_THREADS)
        assert all(hi - lo <= per for lo, hi in runs)
    runs = pg.scan_runs(-(-pg.N2 // pg.TILE))
    assert runs[682] == (2046, 2049) and runs[683] == (2049, 2050) and all(lo == hi == 2050 for lo, hi in runs[684:])
    # a thread that summed its run but rewrote one value too few, or started one late, would show: the exclusive scan by runs
    v = [(i * 37) % 11 for i in range(2050)]
    part = [sum(v[lo:hi]) for lo, hi in runs]
    out = []
    for t, (lo, hi) in enumerate(runs):
        run = sum(part[:t])
        for i in range(lo, hi):
            out.append(run)
            run += v[i]
    assert out == [sum(v[:i]) for i in range(2050)]
