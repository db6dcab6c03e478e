"""`classify_read --ingest device --rows device` through the program: stdout equal to --rows host's, to the stage-03 oracle's and to the
reference goldens, on FASTA and FASTQ, plain and gzip, at a small and at the default block, with and without --bin-reads --gz-out, and
every such run must say that the rows came from the device (a silent fallback does not pass); the fallbacks, which keep stdout; the
format error; the usage errors."""
import os
import re
import subprocess

import pytest

import hast_amd
from tests.conftest import golden_cases, load_case
from tests.test_cli_rs_gpu import FORMAT_MSG, run, stats_of, write_corpus

pytestmark = pytest.mark.gpu
DEV = ["--ingest", "device", "--rows", "device", "--stats"]


@pytest.fixture(scope="module")
def work(tmp_path_factory, oracle_dir):
    """the corpus of the device ingest's test once, with the oracle's rows for each format"""
    d = tmp_path_factory.mktemp("cli_rr")
    n = write_corpus(d)
    want = {}
    for fmt, name in (("fasta", "reads.fa"), ("fastq", "reads.fq")):
        ref = subprocess.run([os.path.join(oracle_dir, "oracle_classify_s03"), "--hap", "h0.mer", "--hap", "h1.mer", "--read", name, "--format", fmt],
                             cwd=d, stdout=subprocess.PIPE, check=True)
        assert len(ref.stdout.splitlines()) == n
        want[fmt] = ref.stdout
    return d, n, want


def rows_stats(stderr):
    m = re.search(rb"\[stats\] rows: route=(\w+) views_on_device=(\d+) views_on_host=(\d+) bytes=(\d+) fallback=(\w+)\n", stderr)
    assert m, stderr[-800:]
    return m.group(1).decode(), int(m.group(2)), int(m.group(3)), int(m.group(4)), m.group(5).decode()


def bin_files(d, sub):
    p = d / sub
    return {f: (p / f).read_bytes() for f in sorted(os.listdir(p))}


@pytest.mark.parametrize("bins", (False, True))
@pytest.mark.parametrize("block", (32768, None))
@pytest.mark.parametrize("gz", (False, True))
@pytest.mark.parametrize("fmt", ("fasta", "fastq"))
def test_device_rows_are_the_host_rows_and_the_oracles(work, fmt, gz, block, bins):
    d, n, want = work
    name = "reads." + ("fa" if fmt == "fasta" else "fq") + (".gz" if gz else "")
    tag = "%s_%d_%s" % (fmt, gz, block)
    env = {"HAST_RS_BLOCK": str(block)} if block else None
    args = ["--read", name, "--format", fmt]
    extra = {}
    for rows in ("host", "device"):
        sub = "bins_%s_%s" % (tag, rows)
        if bins:
            os.makedirs(d / sub, exist_ok=True)
        extra[rows] = ["--bin-reads", "--gz-out", "--bin-dir", sub] if bins else []
    host = run(d, args + ["--ingest", "device", "--rows", "host", "--stats"] + extra["host"], env)
    dev = run(d, args + DEV + extra["device"], env)
    assert host.returncode == 0 and dev.returncode == 0, (host.stderr[-1000:], dev.stderr[-1000:])
    assert host.stdout == want[fmt] and dev.stdout == want[fmt]
    route, on_dev, on_host, nbytes, fallback = rows_stats(dev.stderr)
    tail = len(want[fmt].splitlines(True)[-1]) if fmt == "fastq" else 0         # the FASTQ tail's row is the host's
    assert (route, on_host, fallback) == ("device", 0, "none") and on_dev > 1 and nbytes == len(want[fmt]) - tail, dev.stderr[-600:]
    assert rows_stats(host.stderr) == ("host", 0, 0, 0, "none")
    assert stats_of(dev.stderr)[::2] == ("device", n, "none") and b"WARN" not in dev.stderr
    if block:
        assert on_dev > 50
    if bins:
        a, b = bin_files(d, "bins_%s_host" % tag), bin_files(d, "bins_%s_device" % tag)
        assert len(a) == 3 and a == b


def test_without_the_flag_stderr_has_no_line_on_rows(work):
    d, n, want = work
    r = run(d, ["--read", "reads.fa", "--ingest", "device", "--stats"], {"HAST_RS_BLOCK": "65536"})
    assert r.returncode == 0 and r.stdout == want["fasta"] and b"rows:" not in r.stderr


@pytest.mark.parametrize("case,run_name", golden_cases("s03"))
def test_device_rows_match_s03_reference_golden(golden_workdir, case, run_name):
    meta = load_case(case)["runs"][run_name]
    d = golden_workdir / case
    res = subprocess.run([hast_amd.classify_read_exe()] + meta["argv"] + DEV, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    assert res.stdout == open(d / meta["expected"], "rb").read()
    route, on_dev, on_host, _, fallback = rows_stats(res.stderr)
    assert (route, on_host, fallback) == ("device", 0, "none") and on_dev >= 1


def test_fallbacks_keep_stdout(work):
    d, n, want = work
    for fmt, name in (("fasta", "reads.fa"), ("fastq", "reads.fq.gz")):
        r = run(d, ["--read", name, "--format", fmt] + DEV, {"HAST_RS_BLOCK": "4096"})
        assert r.returncode == 0 and r.stdout == want[fmt], r.stderr[-800:]
        assert stats_of(r.stderr)[4] == "record_too_long" and rows_stats(r.stderr)[0::4] == ("device", "record_too_long") and r.stderr.count(b"WARN") == 1
    r = run(d, ["--read", "reads.fa", "--devices", "0,0"] + DEV)
    assert r.returncode == 0 and r.stdout == want["fasta"], r.stderr[-800:]
    assert rows_stats(r.stderr) == ("host", 0, 0, 0, "several_devices") and r.stderr.count(b"WARN") == 1
    os.mkfifo(d / "pipe.fa")
    writer = subprocess.Popen(["sh", "-c", "cat reads.fa > pipe.fa"], cwd=d)
    r = run(d, ["--read", "pipe.fa"] + DEV)
    assert writer.wait(timeout=60) == 0
    assert r.returncode == 0 and r.stdout == want["fasta"] and r.stderr.count(b"WARN") == 1
    assert rows_stats(r.stderr) == ("device", 0, 0, 0, "not_a_regular_file")
    # a view of records of a few bytes: its rows outgrow the feed's buffer and are formatted here, with no word on stderr but the count
    tiny = b"".join(b">%d\nA\n" % i for i in range(3000))
    (d / "tiny.fa").write_bytes(tiny)
    host = run(d, ["--read", "tiny.fa", "--read", "reads.fa", "--ingest", "host"])
    r = run(d, ["--read", "tiny.fa", "--read", "reads.fa"] + DEV, {"HAST_RS_BLOCK": "32768"})
    assert r.returncode == 0 and host.returncode == 0 and r.stdout == host.stdout and len(r.stdout) > len(want["fasta"]), r.stderr[-800:]
    route, on_dev, on_host, _, fallback = rows_stats(r.stderr)
    assert (route, fallback) == ("device", "none") and on_host >= 1 and on_dev > 50 and b"WARN" not in r.stderr


def test_an_empty_set_has_its_rows_made_on_the_host(work):
    d, n, want = work
    (d / "none.mer").write_bytes(b"")
    args = ["--hap", "h0.mer", "--hap", "none.mer", "--read", "reads.fa", "--thread", "2"]
    exe = hast_amd.classify_read_exe()
    host = subprocess.run([exe] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    dev = subprocess.run([exe] + args + DEV, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert host.returncode == 0 and dev.returncode == 0, (host.stderr[-800:], dev.stderr[-800:])
    assert dev.stdout == host.stdout and len(host.stdout.splitlines()) == n
    assert dev.stderr.count(b"WARN") == 1 and b"--rows device: rows are made on the host (fallback=empty_set)\n" in dev.stderr
    assert rows_stats(dev.stderr) == ("host", 0, 0, 0, "empty_set") and stats_of(dev.stderr)[0] == "device"


def test_the_format_error_ends_the_run_as_before(work):
    d, n, want = work
    lines = (d / "reads.fa").read_bytes().split(b"\n")
    bad = list(lines)
    bad[len(bad) // 2] = b"@" + bad[len(bad) // 2][1:]
    (d / "bad.fa").write_bytes(b"\n".join(bad))
    r = run(d, ["--read", "reads.fa", "--read", "bad.fa"] + DEV, {"HAST_RS_BLOCK": "65536"})
    assert r.returncode == 1 and r.stdout == want["fasta"] and r.stderr.count(FORMAT_MSG["fasta"]) == 1, r.stderr[-500:]
    fq = (d / "reads.fq").read_bytes().split(b"\n")
    at = len(fq) // 8 * 4
    assert fq[at][:1] == b"@"
    fq[at] = b">" + fq[at][1:]
    (d / "bad.fq").write_bytes(b"\n".join(fq))
    r = run(d, ["--read", "reads.fq", "--read", "bad.fq", "--format", "fastq"] + DEV, {"HAST_RS_BLOCK": "65536"})
    assert r.returncode == 1 and r.stdout == want["fastq"] and r.stderr.count(FORMAT_MSG["fastq"]) == 1, r.stderr[-500:]


def test_usage_errors(work):
    d, n, want = work
    for flags in (["--ingest", "device", "--rows", "gpu"], ["--rows", "device"], ["--ingest", "host", "--rows", "device"]):
        r = run(d, ["--read", "reads.fa"] + flags)
        assert r.returncode == 255 and r.stdout == b"" and b"__START__" not in r.stderr and b"--rows host|device" in r.stderr, flags
    r = run(d, ["--read", "reads.fa", "--rows", "host"])                        # the default, said aloud
    assert r.returncode == 0 and r.stdout == want["fasta"]
