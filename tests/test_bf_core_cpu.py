"""Stage 02's per-barcode read count without a GPU: the field rule and the host model (hast_amd/csrc/bf_core.h, bf_host.h) stepped by
tests/native/test_bf_core.cpp, the Python restatement (tests/bf_model.py) and `barcode_freq --count host`, all held to what the
reference's own line wrote for the inputs of tests/golden/barcode_freq/ (rows sorted byte-wise)."""
import gzip
import os
import re
import subprocess

import pytest

import hast_amd
from tests import bf_model
from tests.conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "barcode_freq")
CASES = ("edge_whole", "edge_unterminated_header", "edge_in_line2", "edge_after_header", "empty", "many")


def golden(case, ext):
    with open(os.path.join(GOLDEN, case + ext), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def lib():
    hast_amd.build()
    return hast_amd.lib()


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_native_field_rule_and_streaming_model(tmp_path, sanitize):
    out = str(tmp_path / "test_bf_core")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra"] + (["-fsanitize=address,undefined"] if sanitize else []) + \
          ["-o", out, os.path.join(ROOT, "tests", "native", "test_bf_core.cpp")]
    subprocess.run(cmd, check=True)
    r = subprocess.run([out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith(b"ok ") and b"runtime error" not in r.stderr and b"Sanitizer" not in r.stderr, r.stderr.decode()[-2000:]


@pytest.mark.parametrize("case", CASES)
def test_python_model_reproduces_the_reference(case):
    assert bf_model.rows(bf_model.barcode_freq(golden(case, ".fq"))) == golden(case, ".txt")


def test_many_golden_is_what_it_is_for():
    """3 000 records, one key owning 30 % of them in runs longer than a wave of 64, about 400 keys, some longer than a text record"""
    keys = [line.split(b"#")[1].split(b"/")[0] for line in golden("many", ".fq").split(b"\n")[0::4] if line]
    runs, n = [], 0
    for k in keys + [None]:
        if k == b"0_0_0":
            n += 1
        elif n:
            runs.append(n)
            n = 0
    assert len(keys) == 3000 and sum(runs) == 900 and min(runs) > 64 and len(runs) == 8, (len(keys), runs)
    assert 390 <= len(set(keys)) <= 400 and any(len(k) > 15 for k in keys) and b"" in keys
    assert b"0_0_0\t900\n" in golden("many", ".txt")


def test_rule_table():
    rows = {b"@r#": b"", b"@r##x": b"", b"@r#ab\r": b"ab\r", b"@r#1_2_3/1\tx y": b"1_2_3", b"@r/1": b"1", b"@r#0_0_0/1": b"0_0_0", b"@r#a\0b": b"a\0b",
            b"@r": None, b"": None, b"#": b"", b"@r/1#A_1": b"1"}
    for head, key in rows.items():
        assert bf_model.barcode_freq(head + b"\nAC\n+\nII\n") == ({} if key is None else {key: 1}), head
    # only lines 1, 5, 9, ... count, a file may end inside a record, and nothing is validated
    assert bf_model.barcode_freq(b"x#k\nx#no\nx#no\nx#no\nx#k") == {b"k": 2}
    assert bf_model.barcode_freq(b"x#k\nx#no\nx#no\nx#no\n") == {b"k": 1}
    assert bf_model.barcode_freq(b"") == {} and bf_model.barcode_freq(b"\n") == {}


def run_host(tmp_path, case, gz, block, extra=()):
    name = case + (".fq.gz" if gz else ".fq")
    (tmp_path / name).write_bytes(gzip.compress(golden(case, ".fq"), 6, mtime=0) if gz else golden(case, ".fq"))
    env = dict(os.environ)
    env.pop("HAST_BF_BLOCK", None)
    if block:
        env["HAST_BF_BLOCK"] = str(block)
    return subprocess.run([hast_amd.barcode_freq_exe(), "--count", "host", "--stats", *extra, name], cwd=tmp_path, env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, timeout=120)


def stats_of(stderr, route):
    m = re.search(rb"\[stats\] tally %s: header_lines=(\d+) counted_on_device=(\d+) counted_on_host=(\d+) no_field=(\d+) distinct=(\d+) dictionary_full=([01])\n" % route, stderr)
    assert m, stderr
    return dict(zip(("header_lines", "counted_on_device", "counted_on_host", "no_field", "distinct", "dictionary_full"), map(int, m.groups())))


@pytest.mark.parametrize("block", [0, 100, 300, 700])
@pytest.mark.parametrize("gz", [False, True], ids=["plain", "gz"])
@pytest.mark.parametrize("case", CASES)
def test_host_route_reproduces_the_reference(lib, tmp_path, case, gz, block):
    r = run_host(tmp_path, case, gz, block)
    assert r.returncode == 0, r.stderr
    assert r.stdout == golden(case, ".txt")
    st = stats_of(r.stderr, b"host")
    data = golden(case, ".fq")
    want = bf_model.barcode_freq(data)
    assert st == {"header_lines": sum(want.values()) + bf_model.no_field(data), "counted_on_device": 0, "counted_on_host": sum(want.values()),
                  "no_field": bf_model.no_field(data), "distinct": len(want), "dictionary_full": 0}
    assert re.search(rb"\[stats\] seconds: .*read_phase=", r.stderr)


def test_host_route_zlib_inflate_and_several_inputs(lib, tmp_path):
    """every input is numbered on its own: two inputs that end inside a record count as two streams, not as their concatenation"""
    a, b = golden("edge_in_line2", ".fq"), golden("many", ".fq")
    (tmp_path / "a.fq.gz").write_bytes(gzip.compress(a, 6, mtime=0))
    (tmp_path / "b.fq").write_bytes(b)
    r = subprocess.run([hast_amd.barcode_freq_exe(), "--count", "host", "--inflate", "zlib", "a.fq.gz", "b.fq"], cwd=tmp_path, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr
    want = bf_model.barcode_freq(a)
    for k, c in bf_model.barcode_freq(b).items():
        want[k] = want.get(k, 0) + c
    assert r.stdout == bf_model.rows(want) and r.stdout != bf_model.rows(bf_model.barcode_freq(a + b))
    r = subprocess.run([hast_amd.barcode_freq_exe(), "--count", "host", "-"], cwd=tmp_path, input=b, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and r.stdout == golden("many", ".txt"), r.stderr


def test_program_exit_statuses(lib, tmp_path):
    exe = hast_amd.barcode_freq_exe()
    (tmp_path / "bad.fq.gz").write_bytes(b"\x1f\x8b\x08\x00" + b"\x00" * 40)
    run = lambda *a: subprocess.run([exe, *a], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)  # noqa: E731
    for args in ((), ("--count", "nowhere", "x.fq"), ("--bogus", "x.fq"), ("--max-barcodes", "0", "x.fq"), ("--max-barcodes", "3Q", "x.fq")):
        r = run(*args)
        assert r.returncode == 255 and r.stdout == b"" and b"usage" in r.stderr, (args, r)
    for name in ("missing.fq", "bad.fq.gz"):
        r = run("--count", "host", name)
        assert r.returncode == 2 and r.stdout == b"" and name.encode() in r.stderr, (name, r)
    (tmp_path / "ok.fq").write_bytes(golden("edge_whole", ".fq"))
    with open("/dev/full", "wb") as full:
        r = subprocess.run([exe, "--count", "host", "ok.fq"], cwd=tmp_path, stdout=full, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 3, r


def test_device_route_without_a_gpu_is_a_loud_failure(lib, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    (tmp_path / "ok.fq").write_bytes(golden("edge_whole", ".fq"))
    r = subprocess.run([hast_amd.barcode_freq_exe(), "ok.fq"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 4 and r.stdout == b"", r
