"""Host-only test of the accounting behind hast_sq_feed and hast_rs (hast_amd/csrc/carry_plan.h): tests/native/test_carry_plan.cpp
drives the plan as a sequential model of the feed -- two arrays of exactly the views' size, a toy framer that consumes whole lines,
random inputs in blocks of 64, 65, 100 and 4096 bytes, host and device blocks mixed -- and holds what comes out to what went in
(built with ASAN + UBSAN, run as a process of its own)."""
import os
import re
import subprocess

from tests.conftest import ROOT

SAN = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_carry_plan_against_a_serial_model(tmp_path):
    exe = tmp_path / "test_carry_plan"
    subprocess.run(SAN + ["-o", str(exe), os.path.join(ROOT, "tests", "native", "test_carry_plan.cpp")], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr[-2000:].decode(errors="replace")
    m = re.match(r"ok cases=(\d+) refusals_tried=(\d+)", r.stdout.decode())
    assert m and int(m.group(1)) > 1000 and int(m.group(2)) > 0, r.stdout
