"""The t-mer order of the mod-minimizer (open-closed classes from a 1-KB table in the kernel's LDS) and the overflow mark of
exact-entry sub-buckets, on the host: tests/native/test_tmer_order.cpp."""
import os
import subprocess

from tests.conftest import ROOT


def test_tmer_order_and_overflow_mark(tmp_path):
    exe = tmp_path / "test_tmer_order"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "test_tmer_order.cpp")], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, (r.stdout.decode()[-500:], r.stderr.decode()[-2000:])
    assert r.stdout.startswith(b"ok ")
