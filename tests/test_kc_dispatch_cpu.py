"""The front ends of stage 00's counter that tests/test_kc_geometry_gpu.py claims to run, held against the dispatch as the sources spell it.

launch_kc_count (kc_kernels.hip) picks k_kc_emit4<2..6> or k_kc_count<WT, EMIT> from W = K - m + 1, m, the tile and HAST_KC_EMIT; the kernel
has a one-dword and a 64-bit m-mer branch and, under EMIT, a branch of its own for kc_run_max < W.  This file reads those switches and
bounds out of the sources, restates the dispatch ONCE (front_end below) and asserts that tests/kc_geometry_corpus.py reaches every front end
the sources can produce for 1 <= m <= K <= 32.  If a specialisation is added or a bound moves, the test fails and names the (K, m) the
corpus must gain.  The record geometry (W, kc_rec_off_bits, kc_run_max) comes from kc_common.h itself through tests/native/kc_geometry.cpp."""
import os
import re
import subprocess

import pytest

from tests import kc_geometry_corpus as corpus
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "hast_amd", "csrc")
GAIN = "; tests/kc_geometry_corpus.py must follow (MINIMIZER_PAIRS / cases), or tests/test_kc_geometry_gpu.py no longer runs every front end"


def src(name):
    return open(os.path.join(CSRC, name)).read()


@pytest.fixture(scope="module")
def geometry(tmp_path_factory):
    """{(k, m): (W, kc_rec_off_bits, kc_run_max)} for every 1 <= m <= k <= 32, from the helper"""
    exe = str(tmp_path_factory.mktemp("kc_geometry") / "kc_geometry")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "native", "kc_geometry.cpp")], check=True)
    pairs = [(k, m) for k in range(1, 33) for m in range(1, k + 1)]
    out = subprocess.run([exe] + [str(x) for p in pairs for x in p], check=True, stdout=subprocess.PIPE).stdout.decode().splitlines()
    rows = [tuple(int(x) for x in line.split()) for line in out]
    assert [r[:2] for r in rows] == pairs
    return {r[:2]: r[2:] for r in rows}


def switch_row(name):
    """(name, kind, lo, hi, policy, words) of a row of switches.h's table, as the header spells them"""
    mt = re.search(r'^\s*X\((%s), (\w+), ([^,]+), ([^,]+), (\w+), ("[^"]*"),' % name, src("switches.h"), re.M)
    assert mt, "switches.h has no row %s" % name
    return mt.groups()


class Dispatch:
    """what the sources say"""

    def __init__(self):
        text = src("kc_kernels.hip")
        body = re.search(r"\nhipError_t launch_kc_count\(const KcCountArgs &a, unsigned grid, hipStream_t s\) \{\n(.*?)\n\}\n", text, re.S)
        assert body, "launch_kc_count is no longer where it was" + GAIN
        parts = body.group(1).split("switch (a.k - a.m + 1) {")
        assert len(parts) == 3 and "if (kc_emit4_takes(a)) {" in parts[0], "launch_kc_count: one switch under kc_emit4_takes, one behind it" + GAIN

        def switch(part, launcher):
            block = part.split("\n    }")[0]
            cases = re.findall(r"case (\d+): return %s<(\d+)>\(" % launcher, block)
            default = re.findall(r"default: return %s<(\d+)>\(" % launcher, block)
            assert cases and len(default) == 1 and all(a == b for a, b in cases), (launcher, block)
            assert len(cases) + 1 == len(re.findall(r"\b(?:case \d+|default):", block)), (launcher, block)
            return sorted(int(a) for a, _ in cases), int(default[0])
        self.emit4_cases, self.emit4_default = switch(parts[1], "launch_kc_emit4")
        self.count_cases, self.count_default = switch(parts[2], "launch_kc_count_t")

        takes = re.search(r"static bool kc_emit4_takes\(const KcCountArgs &a\) \{\n(.*?)\n\}\n", text, re.S)
        assert takes, "kc_emit4_takes" + GAIN
        t = takes.group(1)
        assert re.search(r'const bool off = sw::word_is\(sw::HAST_KC_EMIT, "lanes"\);', t) and switch_row("HAST_KC_EMIT")[1::4] == ("Word", '"lanes"'), t
        assert "const int w = a.k - a.m + 1;" in t, t
        ret = re.search(r"return (.*?);", t, re.S).group(1)
        self.takes_terms = [" ".join(x.split()) for x in ret.split("&&")]
        shapes = [r"!off", r"a\.rec_out", r"a\.m == (\d+)", r"w >= (\d+)", r"w <= (\d+)", r"a\.rec_run_max >= \(uint32_t\)w", r"a\.k \+ w \+ 2 <= (\d+)",
                  r"a\.tile_bases % (\d+) == 0", r"a\.tile_bases <= (\d+)", r"a\.rec_chunk >= a\.tile_bases"]
        assert len(self.takes_terms) == len(shapes), "kc_emit4_takes has another condition: %s" % self.takes_terms + GAIN
        num = []
        for term, shape in zip(self.takes_terms, shapes):
            mt = re.fullmatch(shape, term)
            assert mt, "kc_emit4_takes: %r is no longer %r" % (term, shape) + GAIN
            num += [int(g) for g in mt.groups()]
        self.e4_m, self.e4_w_lo, self.e4_w_hi, self.e4_kw, self.e4_tile_mod, self.e4_tile_max = num

        kern = re.search(r"__global__ void __launch_bounds__\(kKcThreads\) k_kc_count\(KcCountArgs a\) \{(.*?)\n\}\n", text, re.S)
        assert kern, "k_kc_count" + GAIN
        k = kern.group(1)
        one = re.findall(r"\n        if \(M <= (\d+)\) \{", k)
        assert len(one) == 1, "k_kc_count phase M: one branch on the m-mer's width" + GAIN
        self.m32 = int(one[0])
        assert "const uint32_t rmax = a.rec_run_max;" in k and len(re.findall(r"if \(rmax < W\) \{", k)) == 1, "k_kc_count: the run cutting of EMIT" + GAIN
        assert "const uint32_t W = WT ? (uint32_t)WT : (uint32_t)(K - M + 1);" in k
        fine = re.search(r"uint32_t kc_rec_fine\(const KcPartGeom &g, unsigned long long rec\) \{.*?\n\}\n", text, re.S)
        assert fine and re.search(r"if \(g\.m <= %d\) \{" % self.m32, fine.group(0)), "kc_rec_fine branches on the m-mer's width where k_kc_count does" + GAIN

        api = src("kc_api.cpp")
        mt = re.search(r"uint32_t tile_bases = (\d+);", api)
        assert mt, "hast_kc::tile_bases"
        self.default_tile = int(mt.group(1))
        mt = re.search(r"uint32_t tile = 0;\s*if \(sw::integer\(sw::HAST_KC_TILE, &tile\)\) c->tile_bases = tile & ~(\d+)u;", api)
        row = switch_row("HAST_KC_TILE")
        assert mt and row[1] == "Int" and row[4] == "Ignore", "HAST_KC_TILE: an integer of the row's [lo, hi], ignored outside it"
        self.tile_lo, self.tile_hi, self.tile_round = int(row[2]), int(row[3]), int(mt.group(1)) + 1
        mt = re.search(r"a\.rec_chunk = (\d+) \* a\.tile_bases;", api)
        assert mt, "rec_chunk"
        self.chunk_tiles = int(mt.group(1))
        assert re.search(r"if \(off \|\| kc_run_max\(c->k, c->m\) == 0 \|\|", api), "part_setup: kc_run_max == 0 keeps the atomic path"
        assert "c->m = default_minimizer_for(k);" in api and "a.rec_run_max = kc_run_max(c->k, c->m);" in api

        host = src("hast_api.cpp")
        mt = re.search(r"int default_minimizer_plain\(int k\) \{ return k <= (\d+) \? k : std::max\((\d+), k - (\d+)\); \}", host)
        assert mt, "default_minimizer_plain is no longer `k <= a ? k : max(b, k - c)`" + GAIN
        self.dm = tuple(int(x) for x in mt.groups())
        row = switch_row("HAST_MINIMIZER")
        assert re.search(r"int v = 0;\s*if \(sw::integer\(sw::HAST_MINIMIZER, &v\) && v <= k\) return v;", host) and row[1:5] == ("Int", "1", "32", "Ignore"), "HAST_MINIMIZER"
        assert "int default_minimizer_for(int k) { return default_minimizer(k); }" in host

    def default_m(self, k):
        a, b, c = self.dm
        return k if k <= a else max(b, k - c)

    def tile_of(self, switches):
        v = int(switches.get("HAST_KC_TILE", 0))
        return v // self.tile_round * self.tile_round if self.tile_lo <= v <= self.tile_hi else self.default_tile

    def front_end(self, geometry, k, m, mode, tile, lanes):
        """THE dispatch, restated once: which kernel instantiation and which of its branches count a stream of this geometry"""
        w, _, rmax = geometry[(k, m)]
        emit = mode == "partition" and rmax > 0
        if (emit and not lanes and m == self.e4_m and self.e4_w_lo <= w <= self.e4_w_hi and rmax >= w and k + w + 2 <= self.e4_kw
                and tile % self.e4_tile_mod == 0 and tile <= self.e4_tile_max and self.chunk_tiles * tile >= tile):
            return "emit4<%d>" % (w if w in self.emit4_cases else self.emit4_default)
        wt = w if w in self.count_cases else self.count_default
        return "count<%d,%s,%s%s>" % (wt, "emit" if emit else "atomic", "m32" if m <= self.m32 else "m64", ",cut" if emit and rmax < w else "")

    def of_case(self, geometry, c):
        return self.front_end(geometry, c.k, corpus.effective_m(c), c.mode, self.tile_of(c.switches), c.switches.get("HAST_KC_EMIT") == "lanes")


@pytest.fixture(scope="module")
def dispatch():
    return Dispatch()


def all_cases():
    return corpus.cases() + corpus.slice_cases()


def test_the_switches_are_the_ones_the_corpus_was_written_for(dispatch):
    d = dispatch
    assert (d.count_cases, d.count_default) == ([1, 6, 8, 9], 0), "launch_kc_count specialises %s" % d.count_cases + GAIN
    assert (d.emit4_cases, d.emit4_default) == ([2, 3, 4, 5], 6), "k_kc_emit4 is instantiated for %s and %d" % (d.emit4_cases, d.emit4_default) + GAIN
    assert (d.e4_m, d.e4_w_lo, d.e4_w_hi, d.e4_kw, d.e4_tile_mod, d.e4_tile_max) == (16, 2, 6, 32, 1024, 16384), d.takes_terms
    assert d.m32 == 16 and d.chunk_tiles == 2
    assert (d.default_tile, d.tile_lo, d.tile_hi, d.tile_round) == (corpus.DEFAULT_TILE, 256, 16384, 32)
    for k in range(1, 33):
        assert corpus.default_m(k) == d.default_m(k), k


def test_corpus_reaches_every_front_end_the_sources_can_produce(dispatch, geometry):
    d = dispatch
    producers = {}
    for k in range(1, 33):
        for m in range(1, k + 1):
            for mode in ("atomic", "partition"):
                for tile in (d.default_tile, d.default_tile + d.tile_round):
                    for lanes in (False, True):
                        producers.setdefault(d.front_end(geometry, k, m, mode, tile, lanes), []).append((k, m, mode, tile, "lanes" if lanes else ""))
    reached = {d.of_case(geometry, c) for c in all_cases()}
    assert reached <= set(producers)
    missing = {name: producers[name][:4] for name in sorted(set(producers) - reached)}
    assert not missing, "no case of the corpus runs %s (front end: some (K, m, mode, tile, HAST_KC_EMIT) that reach it)" % missing + GAIN
    # what 1 <= m <= K <= 32 can produce today, by name: five instantiations x {atomic, emit} x {one dword, 64 bits} x {whole runs, cut
    # runs}, less what no geometry gives (W = 1 is never cut; W = 6 with m <= 16 is K <= 21, where a record has room for 6 windows;
    # W = 8 or 9 with m > 16 is K >= 24, where it has room for 4 at the most), and the five k_kc_emit4
    assert sorted(producers) == sorted(
        ["emit4<%d>" % w for w in (2, 3, 4, 5, 6)] + ["count<%d,atomic,%s>" % (wt, mm) for wt in (0, 1, 6, 8, 9) for mm in ("m32", "m64")] +
        ["count<0,emit,m32>", "count<0,emit,m32,cut>", "count<0,emit,m64>", "count<0,emit,m64,cut>", "count<1,emit,m32>", "count<1,emit,m64>",
         "count<6,emit,m32>", "count<6,emit,m64>", "count<6,emit,m64,cut>", "count<8,emit,m32>", "count<8,emit,m32,cut>", "count<8,emit,m64,cut>",
         "count<9,emit,m32>", "count<9,emit,m32,cut>", "count<9,emit,m64,cut>"]), sorted(producers)


def test_corpus_reaches_what_had_never_run_by_name(dispatch, geometry):
    """the table of front ends that no GPU test ran before tests/test_kc_geometry_gpu.py: each by the case that is there for it"""
    d = dispatch
    by_id = {corpus.case_id(c): c for c in all_cases()}
    assert len(by_id) == len(all_cases()), "two cases share an id"

    def fe(cid):
        return d.of_case(geometry, by_id[cid])
    # k_kc_count<8, false> and <8, true>: K = 23
    assert fe("A-k23-atomic") == "count<8,atomic,m32>" and fe("B-k23-partition") == "count<8,emit,m32,cut>"
    # k_kc_count<9, *> with the one-dword m-mer branch: K = 24
    assert fe("A-k24-atomic") == "count<9,atomic,m32>" and fe("B-k24-partition") == "count<9,emit,m32,cut>"
    assert fe("A-k25-atomic") == "count<9,atomic,m64>" and fe("B-k25-partition") == "count<9,emit,m64,cut>"
    # k_kc_count<0, true>: K = 22; K = 17 .. 20 with HAST_KC_EMIT=lanes; a tile k_kc_emit4 refuses
    assert fe("B-k22-partition") == "count<0,emit,m32,cut>" and fe("A-k22-atomic") == "count<0,atomic,m32>"
    for k in (17, 18, 19, 20):
        assert fe("B-k%d-partition" % k) == "emit4<%d>" % (k - 15) and fe("B-k%d-partition-emitlanes" % k) == "count<0,emit,m32>"
    assert fe("B-k21-partition") == "emit4<6>" and fe("B-k21-partition-emitlanes") == "count<6,emit,m32>"
    for tile in (1056, 288):
        assert fe("B-k19-partition-tile%d" % tile) == "count<0,emit,m32>" and fe("B-k21-partition-tile%d" % tile) == "count<6,emit,m32>"
        assert d.tile_of(by_id["B-k19-partition-tile%d" % tile].switches) == tile          # (a multiple of 32 already: nothing is rounded away)
    # the flush-heavy cases run the cut runs again
    for k in (22, 23, 24):
        assert fe("B-k%d-partition-fresh0-record_mb1" % k).endswith(",m32,cut>")
    # generic W other than 2
    generic_w = {geometry[(c.k, corpus.effective_m(c))][0] for c in all_cases() if d.of_case(geometry, c).startswith("count<0,")}
    assert generic_w >= {2, 3, 4, 5, 7, 10, 11, 12, 13, 14, 15, 17, 21, 32}, sorted(generic_w)
    every_w = {geometry[(k, m)][0] for k, m in corpus.MINIMIZER_PAIRS}
    assert every_w >= {1, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 17, 21, 32}, sorted(every_w)
    # m < 16 under K > 16, in both modes; m > 16 with W other than 9, W = 1 with a 64-bit m-mer among them
    for mode in ("atomic", "partition"):
        assert {(c.k, c.m) for c in all_cases() if c.mode == mode and c.m is not None and c.k > 16 and c.m < 16} >= {(21, 1), (21, 8), (21, 15), (17, 9)}
    assert fe("C-k21m21-partition") == "count<1,emit,m64>" and fe("C-k21m21-atomic") == "count<1,atomic,m64>" and fe("C-k32m32-partition") == "count<1,atomic,m64>"
    assert fe("C-k21m17-partition") == "count<0,emit,m64>" and fe("C-k31m17-partition") == "count<0,atomic,m64>"
    assert {geometry[(c.k, c.m)][0] for c in all_cases() if c.m is not None and c.m > 16} >= {1, 5, 15}
    # kc_run_max == W, < W, == 1 and == 0 in the matrix, and rmax < W with m <= 16
    rel = set()
    for k, m in corpus.MINIMIZER_PAIRS:
        w, _, rmax = geometry[(k, m)]
        rel |= {"zero" if rmax == 0 else "one" if rmax == 1 and w > 1 else "cut" if rmax < w else "whole"}
        if rmax and rmax < w and m <= 16:
            rel.add("cut, m <= 16")
    assert rel == {"zero", "one", "cut", "whole", "cut, m <= 16"}, rel
    assert geometry[(27, 16)][2] == 1 and geometry[(28, 16)][2] == 0 and geometry[(21, 15)][2] == 7 == geometry[(21, 15)][0]
    # the slices: one geometry with cut runs, one with a short m under a long K
    assert [fe(corpus.case_id(c)) for c in corpus.slice_cases()] == ["count<8,atomic,m32>", "count<8,emit,m32,cut>", "count<0,atomic,m32>", "count<0,emit,m32,cut>"]


def test_issue_lists_are_whole():
    cs = corpus.cases()
    assert sorted(c.k for c in cs if c.group == "A") == list(range(1, 33)) and all(c.mode == "atomic" and c.m is None for c in cs if c.group == "A")
    b = [c for c in cs if c.group == "B"]
    assert sorted(c.k for c in b if c.switches == corpus.SMALL) == list(range(1, 28))
    assert sorted(c.k for c in b if c.switches.get("HAST_KC_EMIT") == "lanes") == [17, 18, 19, 20, 21]
    assert sorted((c.k, c.switches["HAST_KC_TILE"]) for c in b if "HAST_KC_TILE" in c.switches) == [(19, "1056"), (19, "288"), (21, "1056"), (21, "288")]
    assert sorted(c.k for c in b if c.switches == corpus.TINY) == [22, 23, 24] and corpus.TINY == {"HAST_KC_RECORD_MB": "1", "HAST_KC_FRESH": "0"}
    assert all(c.mode == "partition" and c.m is None and c.switches.get("HAST_KC_RECORD_MB") in ("8", "1") for c in b)
    want = [(22, 16), (23, 16), (24, 16), (25, 16), (26, 16), (27, 16), (28, 16), (21, 1), (21, 8), (21, 15), (21, 17), (21, 21),
            (17, 9), (16, 8), (16, 9), (12, 7), (8, 1), (2, 1), (26, 18), (32, 32), (32, 16), (32, 1), (31, 17)]
    assert corpus.MINIMIZER_PAIRS[:len(want)] == want
    for mode in ("atomic", "partition"):
        assert [(c.k, c.m) for c in cs if c.group == "C" and c.mode == mode] == corpus.MINIMIZER_PAIRS
    assert corpus.SLICE_PAIRS == [(23, 16), (21, 8)] and corpus.N_SLICES == 3
    for c in cs + corpus.slice_cases():
        env = corpus.environment(c)
        assert set(env) <= set(corpus.CLEARED) and env["HAST_KC_COUNT"] == c.mode and (env.get("HAST_KC_FLUSH") == "sweep") == (c.mode == "partition")
        assert env.get("HAST_MINIMIZER") == (None if c.m is None else str(c.m))


def test_a_record_has_room_for_every_case(geometry):
    """[offset : ob][bases : 2 (K + run - 1)][run - 1 : 5][parent : 1] in 64 bits, a run no longer than the windows of one m-mer occurrence"""
    for c in all_cases():
        k, m = c.k, corpus.effective_m(c)
        w, ob, rmax = geometry[(k, m)]
        assert w == k - m + 1 and rmax <= w and rmax <= 16, (k, m)
        assert (1 << ob) >= w, (k, m)
        if rmax:                                                   # and one more window would not fit, or the occurrence has no more
            assert 2 * (k + rmax - 1) + 6 + ob <= 64, (k, m)
            assert rmax == w or rmax == 16 or 2 * (k + rmax) + 6 + ob > 64, (k, m)
        else:                                                      # no record is ever written: not even one window has room
            assert 2 * k + 6 + ob > 64, (k, m)
