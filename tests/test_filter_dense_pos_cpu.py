"""The dense filter's entries and marks, on the host (tests/native/test_filter_dense_pos.cpp): position sub-buckets invert to
their strings, a window probes what its key files, and filter_dense_file -- the routine k_filter_build runs -- loses no entry in
any filing order while its signed marks send fewer never-filed windows to the table than a constant mark."""
import os
import subprocess

from tests.conftest import ROOT


def test_filter_dense_pos_and_marks(tmp_path):
    exe = tmp_path / "test_filter_dense_pos"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "test_filter_dense_pos.cpp")], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    print(r.stdout.decode())
    assert r.returncode == 0, (r.stdout.decode()[-500:], r.stderr.decode()[-2000:])
    assert r.stdout.splitlines()[-1].startswith(b"ok ")
    assert r.stdout.count(b"(c) order") == 3
