"""Host-only test of a classify launch's plan and of the LDS tile of the two classify kernels (hast_amd/csrc/classify_plan.h: row shape,
reads per tile, dynamic LDS, divisors, grid; hast_amd/csrc/classify_tile.h: where every array of a tile lies, shared by hast_api.cpp,
hast_filter.hip and hast_kernels.hip).  tests/native/test_classify_plan.cpp carries the arithmetic classify_rows did by hand before the
headers existed as its serial model and requires, over a grid of K, minimizer, row length, strictness, filter, LDS override and reads,
the same tile_reads, smem, grid, divisors and refusals; of the layout alone that the arrays are disjoint, aligned and inside bytes() and
every pad at least what its reader reaches; of the divisors that multiply-high divides exactly up to qmax.  It runs plain and under
ASan + UBSan."""
import os
import re
import subprocess

import pytest

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "hast_amd", "csrc")


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def driver(request, tmp_path_factory):
    sanitize = request.param == "asan_ubsan"
    out = str(tmp_path_factory.mktemp("classify_plan") / ("test_classify_plan_san" if sanitize else "test_classify_plan"))
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + (["-fsanitize=address,undefined"] if sanitize else []) + \
          ["-o", out, os.path.join(ROOT, "tests", "native", "test_classify_plan.cpp")]
    subprocess.run(cmd, check=True)
    return out


def test_plans_over_the_grid(driver):
    r = subprocess.run([driver], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and b"runtime error" not in r.stderr and b"Sanitizer" not in r.stderr, r.stderr.decode()[-2000:]
    m = re.search(rb"classify plan ok: (\d+) plans, (\d+) refused, (\d+) divisors stepped", r.stderr)
    assert m and int(m.group(1)) > 10000 and int(m.group(2)) > 0 and int(m.group(3)) > 100, r.stderr.decode()[-2000:]


def test_the_headers_are_host_only_and_the_one_description_of_the_tile():
    """no HIP in either header; the host sizes the tile through the plan, both kernels and rows_are name the layout"""
    read = lambda name: open(os.path.join(SRC, name)).read()
    for name in ("classify_tile.h", "classify_plan.h"):
        text = read(name)
        assert "#include <hip" not in text and "__global__" not in text and "hipError_t" not in text, name
    api, filt, kern, dev = read("hast_api.cpp"), read("hast_filter.hip"), read("hast_kernels.hip"), read("hast_device.h")
    assert "per_read" not in api and "classify_f_queue_bytes" not in api and "classify::plan_for(" in api
    assert "classify_f_queue_bytes" not in filt + kern + dev and "kQCap =" not in filt
    at = filt.index("k_classify_f(ClassifyArgs a) {")
    k_f = filt[at:filt.index("// ---- per-read header", at)]
    for word in ("l1_stride_for(", "FilterTile L{", "L.tile_at()", "L.l1_words()", "L.ws()", "kTileHeadBytes", "kQueueBytes"):
        assert word in k_f, word
    assert "+ 64" not in k_f and "kQCap * 3" not in k_f
    rows_are = filt[filt.index("static bool rows_are("):filt.index("static bool geo_is(")]
    assert "l1_stride_for(" in rows_are and "& ~3" not in rows_are
    at = kern.index("k_classify(ClassifyArgs a) {")
    k_e = kern[at:kern.index("// ---- per-read header", at)]
    for word in ("ExactTile L{", "L.tile_at()", "L.ws()", "L.mh_words()", "kTileHeadBytes"):
        assert word in k_e, word
    assert "+ 16" not in k_e
    # stage 00's count kernel: one statement of where the tile's records begin
    kc = read("kc_kernels.hip")
    assert kc.count("kc_count_rec_at(") == 3 and "(TB + W + 64)" not in kc
