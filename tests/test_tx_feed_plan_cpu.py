"""Host-only test of the reading rule behind `fake_10x --convert device --inflate device` (hast_amd/csrc/tx_feed_plan.h): the paired feed
decides who reads, which mode a step has and when it hands over to the host from the counts the step before left, without looking at
a byte.  tests/native/test_tx_feed_plan.cpp runs that rule as a sequential model of the feed (the conversion is tx::pair_host) and
compares every step -- who read, mode, consumed and carried bytes -- the outputs and the state with a direct re-implementation of the
program's loop over byte vectors.  Built plain and under ASan + UBSan as a stand-alone program."""
import os
import re
import subprocess

import pytest

from tests.conftest import ROOT

SEEDS = (1, 20260, 777)


def build_native(out_dir, sanitize):
    out = os.path.join(str(out_dir), "test_tx_feed_plan_san" if sanitize else "test_tx_feed_plan")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra"] + (["-fsanitize=address,undefined"] if sanitize else []) + \
          ["-o", out, os.path.join(ROOT, "tests", "native", "test_tx_feed_plan.cpp")]
    subprocess.run(cmd, check=True)
    return out


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def driver(request, tmp_path_factory):
    return build_native(tmp_path_factory.mktemp("tx_feed_plan"), request.param == "asan_ubsan")


@pytest.mark.parametrize("seed", SEEDS)
def test_the_feeds_sequence_is_the_programs(driver, seed):
    """12 random cases a seed (every fourth with a record longer than the feed's room): the same steps, outputs and state; a side that
    has to read fits its room unless one of its records does not.  The cases must reach what they are for: steps in which a side
    reads nothing, hand-overs at the inputs' ends, and a carry that outgrows its room."""
    r = subprocess.run([driver, str(seed), "12"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and b"runtime error" not in r.stderr and b"Sanitizer" not in r.stderr, r.stderr.decode()[-2000:]
    m = re.search(rb"cases=(\d+) steps=(\d+) feed_steps=(\d+) side_skipped=(\d+) ends=(\d+) too_long=(\d+)", r.stderr)
    cases, steps, feed_steps, skipped, ends, too_long = (int(x) for x in m.groups())
    assert cases == 12 and feed_steps > 100 and steps > feed_steps
    assert skipped > 0 and ends + too_long == 12 and ends >= 6 and too_long >= 1
