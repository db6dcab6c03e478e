"""`classify_read --ingest device` through the program: stdout equal to the host route's and to the stage-03 oracle's on FASTA and
FASTQ, plain and gzip, at a small and at the default block; the reference goldens; the format errors; the fallbacks."""
import gzip
import os
import random
import re
import subprocess

import pytest

import hast_amd
from tests.conftest import golden_cases, load_case

pytestmark = pytest.mark.gpu
K = 21
FORMAT_MSG = {"fasta": b"fasta detected . ERROR . please use \"--format fastq\". exit ... \n",
              "fastq": b"fasta detected . ERROR . please use \"--format fasta\". exit ... \n"}


def write_corpus(d, seed=4242):
    """the generator of the host route's ingest test (records spanning blocks, multi-line FASTA, junk before the first header, empty
    lines, an unterminated last line, a FASTQ tail record); the longest record is 12 000 bases"""
    rng = random.Random(seed)
    keys = [["".join(rng.choice("ACGT") for _ in range(K)) for _ in range(300)] for _ in range(2)]
    for h in (0, 1):
        (d / ("h%d.mer" % h)).write_text("\n".join(keys[h]) + "\n")
    recs = []
    for i in range(1500):
        L = rng.choice([0, 5, K, 60, 300, 3000, 12000]) if i % 7 else rng.randint(0, 400)
        s = [rng.choice("ACGT") for _ in range(L)]
        for _ in range(rng.randint(0, 1 + L // 200)):
            if L >= K:
                o = rng.randint(0, L - K)
                s[o:o + K] = rng.choice(keys[rng.randint(0, 1)])
        if L and rng.random() < 0.1:
            s[rng.randrange(L)] = rng.choice("Nn")
        recs.append(("r%d some/desc %d" % (i, i), "".join(s)))
    fa = "junk line before any header\nACGT\n"
    for n, s in recs:
        w = rng.choice([60, 70, 1000000])
        fa += ">" + n + "\n" + "".join(s[j:j + w] + "\n" + ("\n" if rng.random() < 0.05 else "") for j in range(0, len(s), w))
    fa += ">last\nACGTACGTACGTACGTACGTACGT\nTTTT"                      # unterminated last line is dropped
    fq = "".join("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)) for n, s in recs) + "@tail x\nACGTACGTACGTACGTACGTACGTA"
    for name, text in (("reads.fa", fa), ("reads.fq", fq)):
        (d / name).write_text(text)
        with gzip.open(d / (name + ".gz"), "wb", compresslevel=1) as f:
            f.write(text.encode())
    return len(recs) + 1


@pytest.fixture(scope="module")
def work(tmp_path_factory, oracle_dir):
    """the corpus once, with the oracle's rows for each format"""
    d = tmp_path_factory.mktemp("cli_rs")
    n = write_corpus(d)
    want = {}
    for fmt, name in (("fasta", "reads.fa"), ("fastq", "reads.fq")):
        ref = subprocess.run([os.path.join(oracle_dir, "oracle_classify_s03"), "--hap", "h0.mer", "--hap", "h1.mer", "--read", name, "--format", fmt],
                             cwd=d, stdout=subprocess.PIPE, check=True)
        assert len(ref.stdout.splitlines()) == n
        want[fmt] = ref.stdout
    return d, n, want


def run(d, args, env=None, timeout=600):
    e = dict(os.environ)
    e.pop("HAST_RS_BLOCK", None)
    e.update(env or {})
    return subprocess.run([hast_amd.classify_read_exe(), "--hap", "h0.mer", "--hap", "h1.mer"] + args, cwd=d, env=e, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, timeout=timeout)


def stats_of(stderr):
    m = re.search(rb"\[stats\] ingest (\w+): blocks_framed=(\d+) records=(\d+) gz_on_device=(\d+) fallback=(\w+)", stderr)
    assert m and re.search(rb"\[stats\] seconds: read=[\d.]+ upload=[\d.]+ kernels=[\d.]+ rows=[\d.]+ read_phase=[\d.]+", stderr), stderr[-600:]
    return m.group(1).decode(), int(m.group(2)), int(m.group(3)), int(m.group(4)), m.group(5).decode()


@pytest.mark.parametrize("block", (32768, None))
@pytest.mark.parametrize("gz", (False, True))
@pytest.mark.parametrize("fmt", ("fasta", "fastq"))
def test_device_ingest_matches_host_ingest_and_oracle(work, fmt, gz, block):
    d, n, want = work
    name = "reads." + ("fa" if fmt == "fasta" else "fq") + (".gz" if gz else "")
    args = ["--read", name, "--format", fmt, "--thread", "4"]
    host = run(d, args + ["--ingest", "host"])
    dev = run(d, args + ["--ingest", "device", "--stats"], {"HAST_RS_BLOCK": str(block)} if block else None)
    assert host.returncode == 0 and dev.returncode == 0, (host.stderr[-1000:], dev.stderr[-1000:])
    assert host.stdout == want[fmt]
    assert dev.stdout == want[fmt]
    route, blocks, records, gz_dev, fallback = stats_of(dev.stderr)
    assert (route, records, fallback) == ("device", n, "none") and blocks > 1, dev.stderr[-600:]
    assert gz_dev == (1 if gz else 0)
    if block:
        assert blocks > 50
    assert b"[stats]" not in host.stderr and b"WARN" not in dev.stderr


@pytest.mark.parametrize("case,run_name", golden_cases("s03"))
def test_device_ingest_matches_s03_reference_golden(golden_workdir, case, run_name):
    meta = load_case(case)["runs"][run_name]
    d = golden_workdir / case
    res = subprocess.run([hast_amd.classify_read_exe()] + meta["argv"] + ["--ingest", "device", "--stats"], cwd=d, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=600)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    assert res.stdout == open(d / meta["expected"], "rb").read()
    assert stats_of(res.stderr)[0] == "device" and stats_of(res.stderr)[4] == "none"


def test_format_errors_end_the_run_as_the_host_route_does(work):
    """exit 1, the reference's message, the rows of the files before and none of the file with the error"""
    d, n, want = work
    lines = (d / "reads.fa").read_bytes().split(b"\n")
    for tag, at in (("first", 0), ("middle", len(lines) // 2), ("last", len(lines) - 2)):
        for c in (b"@", b"+"):
            bad = list(lines)
            bad[at] = c + bad[at][1:]
            (d / ("bad_%s.fa" % tag)).write_bytes(b"\n".join(bad))
            dev = run(d, ["--read", "reads.fa", "--read", "bad_%s.fa" % tag, "--ingest", "device"], {"HAST_RS_BLOCK": "65536"})
            assert dev.returncode == 1 and dev.stdout == want["fasta"] and dev.stderr.count(FORMAT_MSG["fasta"]) == 1, (tag, c, dev.stderr[-500:])
    fq = (d / "reads.fq").read_bytes().split(b"\n")
    for tag, at in (("first", 0), ("middle", len(fq) // 8 * 4), ("tail", len(fq) - 2)):
        bad = list(fq)
        assert bad[at][:1] == b"@"
        bad[at] = b">" + bad[at][1:]
        (d / ("bad_%s.fq" % tag)).write_bytes(b"\n".join(bad))
        dev = run(d, ["--read", "reads.fq", "--read", "bad_%s.fq" % tag, "--format", "fastq", "--ingest", "device"], {"HAST_RS_BLOCK": "65536"})
        assert dev.returncode == 1 and dev.stdout == want["fastq"] and dev.stderr.count(FORMAT_MSG["fastq"]) == 1, (tag, dev.stderr[-500:])
    host = run(d, ["--read", "reads.fq", "--read", "bad_middle.fq", "--format", "fastq"])
    assert host.returncode == 1 and host.stdout == want["fastq"] and host.stderr.count(FORMAT_MSG["fastq"]) == 1


def test_fallbacks_keep_stdout(work):
    d, n, want = work
    for fmt, name in (("fasta", "reads.fa"), ("fastq", "reads.fq.gz")):
        r = run(d, ["--read", name, "--format", fmt, "--ingest", "device", "--stats"], {"HAST_RS_BLOCK": "4096"})
        assert r.returncode == 0 and r.stdout == want[fmt], r.stderr[-800:]
        route, _, records, _, fallback = stats_of(r.stderr)
        assert (route, records, fallback) == ("device", n, "record_too_long") and r.stderr.count(b"WARN") == 1
    r = run(d, ["--read", "reads.fa", "--devices", "0,0", "--ingest", "device", "--stats"])
    assert r.returncode == 0 and r.stdout == want["fasta"], r.stderr[-800:]
    assert stats_of(r.stderr)[0::4] == ("host", "several_devices") and r.stderr.count(b"WARN") == 1
    os.mkfifo(d / "pipe.fa")
    writer = subprocess.Popen(["sh", "-c", "cat reads.fa > pipe.fa"], cwd=d)
    r = run(d, ["--read", "pipe.fa", "--ingest", "device", "--stats"])
    assert writer.wait(timeout=60) == 0
    assert r.returncode == 0 and r.stdout == want["fasta"] and stats_of(r.stderr)[4] == "not_a_regular_file" and r.stderr.count(b"WARN") == 1


def test_damaged_input_and_bad_flags(work):
    d, n, want = work
    whole = (d / "reads.fq.gz").read_bytes()
    (d / "cut.fq.gz").write_bytes(whole[:len(whole) // 2])
    r = run(d, ["--read", "cut.fq.gz", "--format", "fastq", "--ingest", "device"])
    assert r.returncode == 2 and r.stdout == b"", r.stderr[-500:]
    r = run(d, ["--read", "missing.fa", "--ingest", "device"])
    assert r.returncode == 2
    for flags in (["--ingest", "gpu"], ["--ingest", "device", "--block-mb", "0"]):
        r = run(d, ["--read", "reads.fa"] + flags)
        assert r.returncode == 255 and r.stdout == b"" and b"__START__" not in r.stderr, flags
