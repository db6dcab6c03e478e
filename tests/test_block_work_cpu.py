"""Host-only tests of what the programs' host sides share: the work area of the host parsers (hast::BlockWork, hast_amd/csrc/ingest.h)
against a serial model, an input's raw bytes on their way into a carried-block feed (hast::RawBlocks, hast_amd/csrc/raw_blocks.h)
against a fake decoder, and the head logic of the k-mer loader (hast::KmerFiles, hast_amd/csrc/cli_common.h) against a fake table.
The drivers are tests/native/test_block_work.cpp, test_raw_blocks.cpp and test_kmer_files.cpp, built with ASAN + UBSAN and run as
processes of their own."""
import os
import re
import subprocess

from tests.conftest import ROOT

SAN = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread"]


def run_native(tmp_path, name):
    exe = tmp_path / name
    scratch = tmp_path / "inputs"
    scratch.mkdir()
    subprocess.run(SAN + ["-o", str(exe), os.path.join(ROOT, "tests", "native", name + ".cpp"), "-lz"], check=True)
    r = subprocess.run([str(exe), str(scratch)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:].decode(errors="replace")
    return r.stdout.decode()


def test_block_work_against_a_serial_model(tmp_path):
    m = re.match(r"ok cases=(\d+) areas=(\d+) slow_path=(\d+) tiny=(\d+) no_newline=(\d+)", run_native(tmp_path, "test_block_work"))
    assert m and int(m.group(1)) == 20 and all(int(m.group(i)) > 0 for i in (2, 3, 4, 5)), m


def test_raw_blocks_by_every_route(tmp_path):
    m = re.match(r"ok cases=(\d+)", run_native(tmp_path, "test_raw_blocks"))
    assert m and int(m.group(1)) == 17, m


def test_kmer_files_head_logic(tmp_path):
    m = re.match(r"ok cases=(\d+)", run_native(tmp_path, "test_kmer_files"))
    assert m and int(m.group(1)) == 12, m
