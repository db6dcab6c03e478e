"""Host-only tests of what the device step of the stLFR -> 10x conversion decides per record (hast_amd/csrc/tx_plan.h): the map as a
table, the key of a header as the table's key, the plan of a pair and the bytes of both output records.  tests/native/test_tx_plan.cpp
steps these functions as a sequential model of the kernels (tx_kernels.hip) and compares every step with the host model
(tx::pair_host, final = 0) itself; here its outputs are held to what the script wrote (tests/golden/fake10x/)."""
import os
import re
import subprocess

import pytest

from tests import tx_model as tm
from tests.conftest import ROOT

CASES = ("edge", "widths", "long", "fb_value17", "fb_key16", "fb_emptykey")
BLOCKS = (64, 100, 700, 4096, 65536)
DEVICE_OK = ("edge", "widths", "long")


def build_native(out_dir, sanitize):
    """tests/native/test_tx_plan.cpp as a stand-alone program, optionally under ASan + UBSan"""
    out = os.path.join(str(out_dir), "test_tx_plan_san" if sanitize else "test_tx_plan")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra"] + (["-fsanitize=address,undefined"] if sanitize else []) + \
          ["-o", out, os.path.join(ROOT, "tests", "native", "test_tx_plan.cpp")]
    subprocess.run(cmd, check=True)
    return out


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("tx_plan")


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def driver(request, work):
    return build_native(work, request.param == "asan_ubsan")


def clean(r):
    return r.returncode == 0 and b"runtime error" not in r.stderr and b"Sanitizer" not in r.stderr


@pytest.mark.parametrize("block", BLOCKS)
def test_device_model_equals_the_host_model_and_the_script(driver, work, block):
    """every step of mode 0 goes through the sequential device model and through pair_host(final = 0): the driver leaves with 1 at the
    first field or byte that differs; the outputs end to end are the script's"""
    for case in CASES:
        o1, o2 = str(work / "o1.fq"), str(work / "o2.fq")
        args = [str(work / name) for name in ("r1.fq", "r2.fq", "map.txt")]
        for path, name in zip(args, ("r1.fq", "r2.fq", "map.txt")):
            open(path, "wb").write(tm.golden(case, name))
        r = subprocess.run([driver, "-b", str(block)] + args + [o1, o2], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert clean(r), (case, block, r.stderr.decode()[-2000:])
        assert open(o1, "rb").read() == tm.golden(case, "out1.fq") and open(o2, "rb").read() == tm.golden(case, "out2.fq"), (case, block)
        assert r.stdout == tm.banner(*args) + tm.golden(case, "stdout.txt")[len(tm.banner(*tm.GOLDEN_ARGS)):], (case, block)
        m = re.search(rb"steps=(\d+) on_model=(\d+) refused_short=(\d+) over_the_programs_room=(\d+)", r.stderr)
        steps, on_model, refused, over_room = (int(x) for x in m.groups())
        # only widths' six-base records grow past twice their size and 4 KB, and only when a step holds more than 4 KB of them
        assert over_room == (1 if case == "widths" and block == 65536 else 0), (case, block, r.stderr)
        if case in DEVICE_OK:
            assert 1 <= steps - on_model <= 2, (case, block, r.stderr)      # the closing steps are the host model's, nothing else
            if case != "edge":
                assert refused >= 1, (case, block)                         # a room one byte short was refused whole
            if block <= 700 and case != "edge":
                assert steps > 4
        else:
            assert on_model == 0, (case, block)


def test_every_key_of_every_golden_map_is_found_with_its_value(driver, work):
    paths = []
    for case in DEVICE_OK:
        paths.append(str(work / ("map_%s.txt" % case)))
        open(paths[-1], "wb").write(tm.golden(case, "map.txt"))
    r = subprocess.run([driver, "--table"] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert clean(r), r.stderr.decode()[-2000:]
    for case, path in zip(DEVICE_OK, paths):
        assert ("%s: %d keys in " % (path, len(tm.parse_map(tm.golden(case, "map.txt"))))).encode() in r.stderr


def test_a_map_the_device_cannot_take_has_no_table(driver, work):
    path = str(work / "map_fb.txt")
    open(path, "wb").write(tm.golden("fb_key16", "map.txt"))
    r = subprocess.run([driver, "--table", path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 1 and b"key longer than 15 bytes" in r.stderr


def test_key_rules_and_the_table_at_load_one_half(driver):
    """the rows of test_key_rule_table through key_record + table_find; absent keys and header keys of 15 and 16 bytes in a table
    that is exactly half full"""
    r = subprocess.run([driver, "--rules"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert clean(r) and b"rules ok" in r.stderr, r.stderr.decode()[-2000:]
