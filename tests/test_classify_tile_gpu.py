"""The LDS tile of the two classify kernels at the shapes where a wrong offset or pad shows (hast_amd/csrc/classify_tile.h and
classify_plan.h): a small random table, K = 21 and K = 32, probed through the exact table, the sampled filter and the dense filter,
with the tile_lds option at its least (4096: a tile of very few reads), at the default and at its most (163840: 64 reads).  Stage-01
rows of K-1, K, 32, 33 and 150 bases and strict rows (hast_classify_perread_device: reads of 513 and 4097 bases, cut into segment
rows) in batches of three full tiles and one more read, so that the last tile is partial; every read's votes must be the oracle's.
The reads per tile come from the plan itself (tests/native/classify_tile_reads.cpp), not from arithmetic restated here."""
import ctypes as C
import functools
import os
import random
import subprocess

import numpy as np
import pytest

import hast_amd
from hast_amd.binding import make_params
from tests.conftest import ROOT
from tests.test_gpu_parity import _kmer_str, _s03_oracle, built, oracle_from_keys, oracle_votes  # noqa: F401  (built: module fixture)

pytestmark = pytest.mark.gpu

N_KEYS = 3000
TILE_LDS = (4096, 0, 163840)          # 0: the library's own budget
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


@pytest.fixture(scope="module")
def tile_reads(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("classify_tile") / "classify_tile_reads")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "native", "classify_tile_reads.cpp")], check=True)

    @functools.lru_cache(maxsize=None)
    def ask(k, m, read_len, strict, use_filter, t, dense, lds):
        out = subprocess.run([exe] + [str(int(x)) for x in (k, m, read_len, strict, use_filter, t, dense, lds)], check=True,
                             stdout=subprocess.PIPE).stdout.split()
        assert out[2] == b"1", "the plan refuses this shape"
        return int(out[0])
    return ask


def _reads(rng, k, L, n, kmers, strict):
    """n reads of L bases: random, most with a planted key or its reverse complement, some with a byte outside ACGT"""
    seqs = []
    for i in range(n):
        s = [rng.choice("ACGT") for _ in range(L)]
        for _ in range(1 + L // 120):
            if L >= k and rng.random() < 0.8:
                km = rng.choice(kmers)
                o = rng.randint(0, L - k)
                s[o:o + k] = km if rng.random() < 0.5 else "".join(COMP[c] for c in reversed(km))
        if L and i % 7 == 3:
            s[rng.randrange(L)] = rng.choice("NnacgtRYK-") if strict else "N"
        seqs.append("".join(s).encode())
    return seqs


@pytest.mark.parametrize("k,path", [(21, "table"), (21, "sparse"), (21, "dense"), (32, "table"), (32, "sparse")])
def test_votes_at_every_tile_size(built, oracle_lib, monkeypatch, tile_reads, k, path):
    for v in ("HAST_FILTER_EXACT", "HAST_CLASSIFY", "HAST_TILE_LDS", "HAST_MINIMIZER"):
        monkeypatch.delenv(v, raising=False)
    if (k, path) == (21, "sparse"):
        monkeypatch.setenv("HAST_FILTER_EXACT", "once")       # exact entries filed once per strand: the sampled probe with its first level
    rng = random.Random(1000 * k + len(path))
    p = make_params(k, 100, N_KEYS, 1)
    keys = [hast_amd.synth_keys_host(p, h, 0, N_KEYS) for h in (0, 1)]
    lines = [[_kmer_str(x, k) for x in keys[h]] for h in (0, 1)]
    kmers = lines[0] + lines[1]
    oc = oracle_from_keys(oracle_lib, k, keys[0], keys[1])
    oc3 = _s03_oracle(oracle_lib, lines[0], lines[1])
    with hast_amd.Context(k) as ctx:
        if path == "table":
            ctx.set_filter(0)
        else:
            ctx.set_filter(1, 14 if k == 21 else 0)
        ctx.table_reserve(2 * N_KEYS)
        ctx.table_insert_keys(0, keys[0])
        ctx.table_insert_keys(1, keys[1])
        filt, ft, dense = False, 0, False
        if path != "table":
            ctx.filter_build()
            filt, ft, dense = True, ctx.filter_info()[2], ctx.filter_dense()
            assert ctx.filter_mode() in (1, 2) and dense == (path == "dense"), (ctx.filter_mode(), dense)
        else:
            assert ctx.filter_mode() == 0
        m = ctx.minimizer
        hits = 0
        for lds in TILE_LDS:
            ctx.set_option("tile_lds", lds)
            # ---- stage-01 rows: fixed length, whole-read N skip ----
            for L in (k - 1, k, 32, 33, 150):
                tr = tile_reads(k, m, L, 0, filt, ft, dense, lds)
                n = 3 * tr + 1
                bases = np.frombuffer(b"".join(_reads(rng, k, L, n, kmers, False)), dtype=np.uint8).copy()
                off = np.arange(n + 1, dtype=np.uint64) * L
                want = oracle_votes(oracle_lib, oc, bases, off)
                d_b, d_v = ctx.to_device(bases), ctx.alloc(n * 8)
                ctx.memset(d_v, 0xEE, n * 8)
                ctx.classify_device(d_b, bases.size, n, L, d_votes=d_v)
                ctx.sync()
                got = ctx.to_host(d_v, (n, 2), np.uint32)
                ctx.free(d_b)
                ctx.free(d_v)
                assert np.array_equal(got, want), (lds, L, tr, int((got != want).any(axis=1).sum()))
                assert L < k or int(want.sum()) > 0 or n < 8, (lds, L)
                hits += int(want.sum())
            # ---- strict rows: segments of 482 windows of reads of 513 and 4097 bases ----
            tr = tile_reads(k, m, 482 + k - 1, 1, filt, ft, dense, lds)
            n = 3 * tr + 1
            seqs = [s for i in range(n) for s in _reads(rng, k, 4097 if i % 4 == 1 else 513, 1, kmers, True)]
            lens = np.array([len(s) for s in seqs], dtype=np.uint64)
            off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
            bases = np.frombuffer(b"".join(seqs), dtype=np.uint8).copy()
            want = np.zeros((n, 2), np.uint32)
            h0, h1 = C.c_uint32(), C.c_uint32()
            for i, sq in enumerate(seqs):
                oracle_lib.ho_s03_read_hits(oc3, sq, len(sq), C.byref(h0), C.byref(h1))
                want[i] = (h0.value, h1.value)
            d_b, d_o, d_v = ctx.to_device(bases), ctx.to_device(off), ctx.alloc(n * 8)
            ctx.memset(d_v, 0xEE, n * 8)
            ctx.classify_perread_device(d_b, bases.size, d_o, n, d_v)
            ctx.sync()
            got = ctx.to_host(d_v, (n, 2), np.uint32)
            for d in (d_b, d_o, d_v):
                ctx.free(d)
            assert np.array_equal(got, want), (lds, "strict", tr, int((got != want).any(axis=1).sum()))
            assert int(want.sum()) > 0
        assert hits > 0
    oracle_lib.ho_free(oc)
    oracle_lib.ho_s03_free(oc3)
