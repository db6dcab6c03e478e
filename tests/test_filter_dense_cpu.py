"""Dense filing of exact filter entries, on the host (tests/native/test_filter_dense.cpp): the geometry rule, the inversion of
every (block, sub-bucket, entry) a dense insert files, and the blocks per read of the probe's fixed grid."""
import os
import subprocess

from tests.conftest import ROOT


def test_filter_dense_placement(tmp_path):
    exe = tmp_path / "test_filter_dense"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "test_filter_dense.cpp")], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, (r.stdout.decode()[-500:], r.stderr.decode()[-2000:])
    assert r.stdout.startswith(b"ok ")
