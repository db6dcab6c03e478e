"""Stage 00's counter at every K and minimizer length its front ends dispatch on (tests/kc_geometry_corpus.py; the claim that the list
reaches every front end is held against the sources by tests/test_kc_dispatch_cpu.py).

Counts per canonical k-mer do not depend on the minimizer length, so the oracle (ho_s00_*) is the reference for every case: distinct and
total counts, the whole histogram, selection sizes, the sorted selections as text byte for byte -- then a further stretch counted in after
the table has been read, and everything compared again.  Whether a counter is partitioned comes from kc_common.h itself
(tests/native/kc_geometry.cpp).  A full table is a failure here: the table holds every case's keys ten times over, asserted on the oracle."""
import functools
import os
import subprocess

import numpy as np
import pytest

import hast_amd
from hast_amd import KmerCounter
from tests import kc_geometry_corpus as corpus
from tests.conftest import ROOT
from tests.test_kc_gpu import built, key_text, oracle_histo, oracle_select, oracle_table  # noqa: F401  (built: module fixture)

pytestmark = pytest.mark.gpu

BOUNDS = [(1, 1 << 30), (2, 5), (1, 1)]


@pytest.fixture(scope="module")
def geometry(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kc_geometry") / "kc_geometry")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "native", "kc_geometry.cpp")], check=True)

    @functools.lru_cache(maxsize=None)
    def ask(k, m):
        out = subprocess.run([exe, str(k), str(m)], check=True, stdout=subprocess.PIPE).stdout.split()
        assert (int(out[0]), int(out[1])) == (k, m)
        return dict(w=int(out[2]), ob=int(out[3]), rmax=int(out[4]))
    return ask


@pytest.fixture(scope="module")
def reference(oracle_lib):
    """the streams of a (K, m) and what the oracle says of them; cases of one (K, m) follow each other, so two entries are kept"""
    o = oracle_lib

    @functools.lru_cache(maxsize=2)
    def of(k, m):
        pat, mat, shared, more = corpus.streams(k, m)
        c = oracle_table(o, k, [(0, pat), (0, shared), (1, mat), (1, shared)])
        sel = {(p, b): oracle_select(o, c, p, *b) for p in (0, 1) for b in BOUNDS}
        ref = dict(streams=(pat, mat, shared, more), sizes={pb: v.size for pb, v in sel.items()},
                   stats=(tuple(o.ho_s00_distinct(c, p) for p in (0, 1)), tuple(o.ho_s00_total(c, p) for p in (0, 1))),
                   histo=[oracle_histo(o, c, p) for p in (0, 1)],
                   keys=[np.sort(np.concatenate([sel[(p, b)] for b in BOUNDS])) for p in (0, 1)])
        ref["text"] = [key_text(o, ref["keys"][p], k) for p in (0, 1)]
        o.ho_s00_add_stream(c, 1, more.ctypes.data, more.size)
        ref["stats_more"] = (tuple(o.ho_s00_distinct(c, p) for p in (0, 1)), tuple(o.ho_s00_total(c, p) for p in (0, 1)))
        ref["histo_more"] = [oracle_histo(o, c, p) for p in (0, 1)]
        o.ho_s00_free(c)
        # the keys of the table = the distinct k-mers of both parents' streams taken as one (a selection leaves out what both have)
        c = oracle_table(o, k, [(0, pat), (0, shared), (0, mat)])
        ref["union"] = int(o.ho_s00_distinct(c, 0))
        o.ho_s00_add_stream(c, 0, more.ctypes.data, more.size)
        ref["union_more"] = int(o.ho_s00_distinct(c, 0))
        o.ho_s00_free(c)
        return ref
    return of


def set_environment(monkeypatch, case):
    for name in corpus.CLEARED:
        monkeypatch.delenv(name, raising=False)
    for name, value in corpus.environment(case).items():
        monkeypatch.setenv(name, value)


CASES = sorted(corpus.cases(), key=lambda c: (c.k, corpus.effective_m(c)))       # (stable: the cases of one (K, m) side by side)


@pytest.mark.parametrize("case", CASES, ids=corpus.case_id)
def test_counts_at_every_geometry_equal_oracle(built, oracle_lib, monkeypatch, geometry, reference, case):
    k, m = case.k, corpus.effective_m(case)
    ref = reference(k, m)
    pat, mat, shared, more = ref["streams"]
    # the table holds this case's keys ten times over: a "table full" below is a wrong answer, never an outcome
    assert 0 < ref["union"] <= ref["union_more"] and ref["union_more"] * 10 < corpus.TABLE_SLOTS, (ref["union_more"], corpus.TABLE_SLOTS)
    set_environment(monkeypatch, case)
    partitioned = case.mode == "partition" and geometry(k, m)["rmax"] > 0
    with KmerCounter(k, table_bytes=corpus.TABLE_BYTES) as kc:
        assert kc.stats()["capacity"] == corpus.TABLE_SLOTS
        assert kc.partition_info()["partitioned"] == partitioned, (kc.partition_info(), geometry(k, m))
        kc.count(0, pat)
        kc.count(1, mat)
        for p in (0, 1):
            kc.count(p, shared)
        kc.sync()
        st = kc.stats()
        assert (st["distinct"], st["total"]) == ref["stats"]
        assert st["keys"] == ref["union"]
        for p in (0, 1):
            assert np.array_equal(kc.histo(p), ref["histo"][p]), p
        for b in BOUNDS:
            assert [kc.select(p, *b) for p in (0, 1)] == [ref["sizes"][(p, b)] for p in (0, 1)], b
        # counting goes on after the table has been read
        kc.count(1, more)
        st = kc.stats()
        assert (st["distinct"], st["total"]) == ref["stats_more"]
        assert st["keys"] == ref["union_more"]
        for p in (0, 1):
            assert np.array_equal(kc.histo(p), ref["histo_more"][p]), p
        info = kc.partition_info()
        print(corpus.case_id(case), geometry(k, m), info)
        assert info["partitioned"] == partitioned, info
        if partitioned:
            assert info["flushes"] >= 1 and info["records"] > 0, info
            if case.switches.get("HAST_KC_RECORD_MB") == "1":
                assert info["flushes"] >= 2, info
        else:
            assert info["flushes"] == 0 and info["records"] == 0, info
        # the selections (made before the further stretch), sorted: the oracle's keys as text, byte for byte
        kc.release_table()
        for p in (0, 1):
            n = kc.selection_sort(p)
            assert n == ref["keys"][p].size
            assert kc.selection_text(p, 0, n) == ref["text"][p], p


@pytest.mark.parametrize("case", corpus.slice_cases(), ids=corpus.case_id)
def test_slices_at_a_geometry_of_their_own(built, oracle_lib, monkeypatch, geometry, reference, case):
    """set_slice(s, 3) for s = 0, 1, 2 at a non-default geometry: the slices' histograms and distinct counts sum to the oracle's, each slice
    holds some keys but not all, and the selections of the three slices together are the oracle's"""
    k, m = case.k, case.m
    ref = reference(k, m)
    pat, mat, shared, _ = ref["streams"]
    assert 0 < ref["union"] * 10 < corpus.TABLE_SLOTS
    set_environment(monkeypatch, case)
    partitioned = case.mode == "partition" and geometry(k, m)["rmax"] > 0
    with KmerCounter(k, table_bytes=corpus.TABLE_BYTES) as kc:
        assert kc.partition_info()["partitioned"] == partitioned
        h = [np.zeros(hast_amd.KC_HISTO_HIGH + 2, dtype=np.uint64) for _ in (0, 1)]
        distinct, total, keys = [0, 0], [0, 0], 0
        for s in range(corpus.N_SLICES):
            kc.set_slice(s, corpus.N_SLICES)
            kc.count(0, pat)
            kc.count(1, mat)
            for p in (0, 1):
                kc.count(p, shared)
            kc.sync()
            st = kc.stats()
            assert 0 < st["keys"] < ref["union"], (s, st)
            keys += st["keys"]
            for p in (0, 1):
                kc.histo(p, into=h[p])
                distinct[p] += st["distinct"][p]
                total[p] += st["total"][p]
                kc.select(p, *BOUNDS[0])
        assert keys == ref["union"]
        assert (tuple(distinct), tuple(total)) == ref["stats"]
        for p in (0, 1):
            assert np.array_equal(h[p], ref["histo"][p]), p
        if partitioned:
            info = kc.partition_info()
            assert info["flushes"] >= 1 and info["records"] > 0, info
        kc.release_table()
        for p in (0, 1):
            want = oracle_keys_text(oracle_lib, ref, p, k)
            n = kc.selection_sort(p)
            assert n == ref["sizes"][(p, BOUNDS[0])]
            assert kc.selection_text(p, 0, n) == want, p


def oracle_keys_text(o, ref, p, k):
    """every key of parent p once, sorted, as text: ref["keys"] holds the three selections together, so each key once and again for every
    further bound it falls under -- the distinct keys are the selection with the widest bounds"""
    return key_text(o, np.unique(ref["keys"][p]), k)
