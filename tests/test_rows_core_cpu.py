"""Host-only test of the output table's rules (hast_amd/csrc/rows_core.h): the host model of rows_host.h, stepped by
tests/native/test_rows_core.cpp, against the independent model of tests/rows_model.py over every case of tests/rows_corpus.py; the
128-bit key's order against the order of bytes on all pairs of a few hundred texts; row_hap against hast_get_hap of the library.
Once plain and once under ASan + UBSan."""
import os
import struct
import subprocess

import numpy as np
import pytest

import hast_amd
from tests import rows_corpus as rc
from tests import rows_model as rm
from tests.conftest import ROOT


def build_native(out_dir, sanitize=False):
    out = os.path.join(str(out_dir), "test_rows_core_san" if sanitize else "test_rows_core")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra"] + (["-fsanitize=address,undefined"] if sanitize else []) + \
          ["-o", out, os.path.join(ROOT, "tests", "native", "test_rows_core.cpp")]
    subprocess.run(cmd, check=True)
    return out


def case_bytes(case):
    _, names, c0, c1, n0, n1, w0, w1 = case
    return struct.pack("<QQQdd", len(names), n0, n1, w0, w1) + rc.text16(names).tobytes() + rc.counts4(c0, c1).tobytes()


@pytest.fixture(scope="module")
def cases():
    return [(c, rm.build(*c[1:])) for c in rc.cases()]


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def results(request, cases, tmp_path_factory):
    """the driver's files for every case"""
    work = tmp_path_factory.mktemp("rows_core_" + request.param)
    driver = build_native(work, sanitize=request.param == "asan_ubsan")
    paths = []
    for case, _ in cases:
        p = str(work / case[0])
        with open(p, "wb") as f:
            f.write(case_bytes(case))
        paths.append(p)
    r = subprocess.run([driver] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"runtime error" not in r.stderr and b"Sanitizer" not in r.stderr, r.stderr.decode()[-2000:]
    flags = {line.split()[0]: tuple(int(x) for x in line.split()[1:]) for line in r.stdout.decode().splitlines()}
    return paths, flags


def test_the_host_model_is_the_python_model(cases, results):
    paths, flags = results
    seen_sep, seen_past = set(), set()
    for (case, want), p in zip(cases, paths):
        name = case[0]
        assert open(p + ".table", "rb").read() == want.table, name
        for l in range(3):
            assert open(p + ".list%d" % (l + 1), "rb").read() == want.lists[l], (name, l)
        assert list(open(p + ".cls", "rb").read()) == want.cls, name
        assert np.fromfile(p + ".order", dtype=np.uint32).tolist() == want.order, name
        assert flags[p] == (int(want.any_sep), int(want.past_int)), name
        seen_sep.add(want.any_sep)
        seen_past.add(want.past_int)
    assert seen_sep == {False, True} and seen_past == {False, True}


def test_the_key_orders_texts_as_bytes_order_them(cases, results):
    """all pairs of the special names (a few hundred): key(a) < key(b) exactly when a < b as bytes"""
    paths, _ = results
    case, p = next((c, p) for (c, _), p in zip(cases, paths) if c[0] == "n700_weighted_sep")
    names = case[1][:420]
    keys = [tuple(int(x, 16) for x in line.split()) for line in open(p + ".keys").read().splitlines()][:420]
    assert len(names) == 420 and all(k[0] < 2 ** 64 and k[1] < 2 ** 64 for k in keys)
    n_second_word = 0
    for i, a in enumerate(names):
        for j, b in enumerate(names):
            assert (keys[i] < keys[j]) == (a < b) and (keys[i] == keys[j]) == (i == j), (a, b, keys[i], keys[j])
            n_second_word += a[:8] == b[:8] and i != j and len(a) >= 8
    assert n_second_word > 500


def test_row_hap_is_hast_get_hap(cases, results):
    paths, _ = results
    calls = set()
    for (case, _), p in zip(cases, paths):
        _, names, c0, c1, n0, n1, w0, w1 = case
        got = [int(x) for x in open(p + ".haps").read().split()]
        assert len(got) == len(names)
        for t, a, b, g in zip(names[:3000], c0, c1, got):
            want = hast_amd.get_hap(t, a, b, n0, n1, w0, w1)
            assert g == want == rm.hap(t, a, b, n0, n1, w0, w1), (case[0], t, a, b, g, want)
            calls.add(g)
    assert calls == {-1, 0, 1}
