"""Host-only test of the partitioned commit's plan (hast_amd/csrc/commit_plan.h: bins, capacity, the layout of the scratch that the
allocator in hast_api.cpp and the launcher in hast_kernels.hip share).  tests/native/test_commit_plan.cpp checks, over a grid of reads,
barcodes and span overrides, that the regions are disjoint, aligned and inside the scratch, that a bin's two counters share a 128-byte
line of their own, and that usable() refuses votes over 255, 2^31 reads and bins whose sums would pass 32 bits; it runs plain and
under ASan + UBSan."""
import os
import re
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def driver(request, tmp_path_factory):
    sanitize = request.param == "asan_ubsan"
    out = str(tmp_path_factory.mktemp("commit_plan") / ("test_commit_plan_san" if sanitize else "test_commit_plan"))
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + (["-fsanitize=address,undefined"] if sanitize else []) + \
          ["-o", out, os.path.join(ROOT, "tests", "native", "test_commit_plan.cpp")]
    subprocess.run(cmd, check=True)
    return out


def test_plans_over_the_grid(driver):
    r = subprocess.run([driver], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and b"runtime error" not in r.stderr and b"Sanitizer" not in r.stderr, r.stderr.decode()[-2000:]
    m = re.search(rb"commit plan ok: (\d+) plans", r.stderr)
    assert m and int(m.group(1)) > 2000, r.stderr.decode()[-2000:]


def test_the_plan_header_is_host_only_and_the_one_description_of_the_scratch():
    """no HIP in the header; the launcher and the allocator take their offsets and sizes from it, not from arithmetic of their own"""
    src = os.path.join(ROOT, "hast_amd", "csrc")
    plan = open(os.path.join(src, "commit_plan.h")).read()
    assert "#include <hip" not in plan and "__global__" not in plan and "__device__" not in plan
    kernels, api = open(os.path.join(src, "hast_kernels.hip")).read(), open(os.path.join(src, "hast_api.cpp")).read()
    launcher = kernels[kernels.index("hipError_t launch_commit_partitioned("):kernels.index("hipError_t launch_scan_n(")]
    for field in ("over_n_at", "lines_at", "recs_at", "over_ids_at", "over_votes_at", "lds_partition", "lds_bins"):
        assert "pl." + field in launcher, field
    assert "hipMemsetAsync" not in launcher and "hipFuncSetAttribute" not in launcher
    assert "commit::plan_for(" in api and "commit::usable(" in api
