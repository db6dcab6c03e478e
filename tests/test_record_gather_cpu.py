"""Host-only test of the wave-per-record gather the routing, read-name and stage-00 FASTQ kernels run (hast_amd/csrc/record_gather.h:
k_route_copy, k_rs_names, k_sq_copy): tests/native/test_record_gather.cpp steps the lane function over every (wave, lane) of its tiles,
in both orders and with both policies, against a serial concatenation, with buffers exactly as large as the contract allows (built with
ASAN + UBSAN, run as a process of its own)."""
import os
import re
import subprocess

from tests.conftest import ROOT

SAN = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_record_gather_lane_by_lane(tmp_path):
    exe = tmp_path / "test_record_gather"
    subprocess.run(SAN + ["-o", str(exe), os.path.join(ROOT, "tests", "native", "test_record_gather.cpp")], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr[-2000:].decode(errors="replace")
    m = re.match(r"ok cases=(\d+) lane_calls=(\d+)", r.stdout.decode())
    assert m and int(m.group(1)) > 800 and int(m.group(2)) > 0, r.stdout
