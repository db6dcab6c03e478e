"""Host-only test of the span copy the FASTA and read-bin kernels run (hast_amd/csrc/span_copy.h: k_rs_copy, k_sqfa_copy, k_rb_copy):
tests/native/test_span_copy.cpp steps the lane function over every (tile, lane) of its cases, in both orders, against a serial
concatenation, with buffers exactly as large as the contract allows (built with ASAN + UBSAN, run as a process of its own)."""
import os
import re
import subprocess

from tests.conftest import ROOT

SAN = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_span_copy_lane_by_lane(tmp_path):
    exe = tmp_path / "test_span_copy"
    subprocess.run(SAN + ["-o", str(exe), os.path.join(ROOT, "tests", "native", "test_span_copy.cpp")], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr[-2000:].decode(errors="replace")
    m = re.match(r"ok cases=(\d+) lane_calls=(\d+)", r.stdout.decode())
    assert m and int(m.group(1)) > 1000 and int(m.group(2)) > 0, r.stdout
