"""Host-only test of the CLI's block feed (hast_amd/csrc/fq_feed.h) against a fake stream: compiled with ThreadSanitizer."""
import os
import subprocess

from tests.conftest import ROOT


def test_fq_feed_protocol_under_tsan(tmp_path):
    exe = tmp_path / "test_fq_feed"
    scratch = tmp_path / "inputs"
    scratch.mkdir()
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=thread", "-pthread", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "test_fq_feed.cpp"), "-lz"], check=True)
    r = subprocess.run([str(exe), str(scratch)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"ThreadSanitizer" not in r.stderr
    assert r.stdout.startswith(b"ok ")
