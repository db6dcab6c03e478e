"""`classify_read --bin-reads` through the program: on FASTA and FASTQ, plain and gzip input, plain and gzip output, at a small and
at the default block, both ingests leave the same files, and every file (after `gzip -dc` where it applies) is the run of
tests/rb_model.py for the classes in the stage-03 oracle's rows; stdout is what it is without the flag; the stats line; the fallback
that reads a file again; the format error; the usage errors; --bin-dir."""
import gzip
import os
import random
import re
import subprocess

import pytest

import hast_amd
from tests import rb_model as rb
from tests import rs_corpus as rc

pytestmark = pytest.mark.gpu
K = 21
EXT = {"fasta": ("fa", rc.FASTA), "fastq": ("fq", rc.FASTQ)}
FORMAT_MSG = {"fasta": b"fasta detected . ERROR . please use \"--format fastq\". exit ... \n",
              "fastq": b"fasta detected . ERROR . please use \"--format fasta\". exit ... \n"}


def write_corpus(d, seed=777):
    """1200 records from empty to 12 000 bases with keys of two sets of different sizes planted; FASTA over 60 and 70 columns and on
    one line, with junk in front of the first header, blank lines and an unterminated last line; FASTQ with a tail record; each also
    as .gz"""
    rng = random.Random(seed)
    keys = [["".join(rng.choice("ACGT") for _ in range(K)) for _ in range(n)] for n in (300, 280)]
    for h in (0, 1):
        (d / ("h%d.mer" % h)).write_text("\n".join(keys[h]) + "\n")
    recs = []
    for i in range(1200):
        L = rng.choice([0, 5, K, 60, 300, 3000, 12000]) if i % 5 else rng.randint(0, 400)
        s = [rng.choice("ACGT") for _ in range(L)]
        for _ in range(rng.randint(0, 1 + L // 300)):
            if L >= K:
                o = rng.randint(0, L - K)
                s[o:o + K] = rng.choice(keys[rng.randint(0, 1)])
        recs.append(("r%d some/desc %d" % (i, i), "".join(s)))
    fa = "junk line before any header\nACGT\n\n"
    for n, s in recs:
        w = rng.choice([60, 70, 1000000])
        fa += ">" + n + "\n" + "".join(s[j:j + w] + "\n" + ("\n" if rng.random() < 0.05 else "") for j in range(0, len(s), w))
    fa += ">last\n" + keys[1][0] + "ACG\nTTTT"                          # the unterminated last line is dropped
    fq = "".join("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)) for n, s in recs) + "@tail x\n" + keys[0][0] + "ACGT"
    for name, text in (("reads.fa", fa), ("reads.fq", fq)):
        (d / name).write_text(text)
        with gzip.open(d / (name + ".gz"), "wb", compresslevel=1) as f:
            f.write(text.encode())
    return len(recs) + 1


@pytest.fixture(scope="module")
def work(tmp_path_factory, oracle_dir):
    """the corpus once; per format the oracle's rows and the model's runs for the classes in them"""
    d = tmp_path_factory.mktemp("cli_bins")
    n = write_corpus(d)
    want = {}
    for fmt, (ext, code) in EXT.items():
        ref = subprocess.run([os.path.join(oracle_dir, "oracle_classify_s03"), "--hap", "h0.mer", "--hap", "h1.mer", "--read", "reads." + ext, "--format", fmt],
                             cwd=d, stdout=subprocess.PIPE, check=True)
        rows = ref.stdout.splitlines()
        assert len(rows) == n
        classes = [rb.CLASSES.index(r.split(b"\t")[-2].decode()) for r in rows]
        data = (d / ("reads." + ext)).read_bytes()
        runs, count = rb.runs_by_class(code, data, classes)
        assert min(count) > 20 and sum(count) == n
        tail = len(rb.extents(code, data)[-1]) if fmt == "fastq" else 0
        want[fmt] = (ref.stdout, runs, count, tail)
    return d, n, want, {}


def run(d, args, env=None, timeout=600):
    e = dict(os.environ)
    e.pop("HAST_RS_BLOCK", None)
    e.update(env or {})
    return subprocess.run([hast_amd.classify_read_exe(), "--hap", "h0.mer", "--hap", "h1.mer"] + args, cwd=d, env=e, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, timeout=timeout)


def new_dir(d, tag):
    out = d / tag
    out.mkdir()
    return out


def files_of(out):
    """{name: plain bytes} of a --bin-dir; a .gz file through `gzip -dc`"""
    got = {}
    for name in sorted(os.listdir(out)):
        p = os.path.join(out, name)
        got[name] = subprocess.run(["gzip", "-dc", p], stdout=subprocess.PIPE, check=True).stdout if name.endswith(".gz") else open(p, "rb").read()
    return got


def expected_files(base, fmt, gz_out, runs):
    return {"%s.%s.%s%s" % (base, rb.CLASSES[c], fmt, ".gz" if gz_out else ""): runs[c] for c in range(3) if runs[c]}


def bins_of(stderr):
    m = re.search(rb"\[stats\] bins: haplotype0=(\d+) haplotype1=(\d+) ambiguous=(\d+) bytes_on_device=(\d+) bytes_on_host=(\d+) gz=([01])\n", stderr)
    assert m, stderr[-600:]
    assert re.search(rb"\[stats\] ingest (\w+): blocks_framed=(\d+) records=(\d+) gz_on_device=(\d+) fallback=(\w+)\n", stderr)
    assert re.search(rb"\[stats\] seconds: read=[\d.]+ upload=[\d.]+ kernels=[\d.]+ rows=[\d.]+ read_phase=[\d.]+\n", stderr)
    return [int(x) for x in m.groups()]


@pytest.mark.parametrize("block", (32768, None))
@pytest.mark.parametrize("gz_out", (False, True))
@pytest.mark.parametrize("gz_in", (False, True))
@pytest.mark.parametrize("fmt", ("fasta", "fastq"))
def test_both_ingests_leave_the_models_files(work, fmt, gz_in, gz_out, block):
    d, n, want, cache = work
    rows, runs, count, tail = want[fmt]
    base = "reads." + EXT[fmt][0]
    name = base + (".gz" if gz_in else "")
    args = ["--read", name, "--format", fmt, "--thread", "4"]
    env = {"HAST_RS_BLOCK": str(block)} if block else None
    flags = ["--bin-reads"] + (["--gz-out"] if gz_out else [])
    tag = "%s_%d_%d_%s" % (fmt, gz_in, gz_out, block)
    # (the runs that do not depend on every parameter are made once)
    if ("off", fmt, gz_in, block) not in cache:
        cache[("off", fmt, gz_in, block)] = run(d, args + ["--ingest", "device"], env)
    if ("host", fmt, gz_in, gz_out) not in cache:
        out = new_dir(d, "host_" + tag)
        cache[("host", fmt, gz_in, gz_out)] = (run(d, args + ["--ingest", "host", "--stats", "--bin-dir", str(out)] + flags), out)
    off = cache[("off", fmt, gz_in, block)]
    host, host_out = cache[("host", fmt, gz_in, gz_out)]
    dev_out = new_dir(d, "dev_" + tag)
    dev = run(d, args + ["--ingest", "device", "--stats", "--bin-dir", str(dev_out)] + flags, env)
    assert off.returncode == 0 and host.returncode == 0 and dev.returncode == 0, (off.stderr[-600:], host.stderr[-600:], dev.stderr[-600:])
    assert off.stdout == rows and dev.stdout == off.stdout and host.stdout == rows
    assert b"[stats]" not in off.stderr and b"WARN" not in dev.stderr
    expect = expected_files(base, fmt, gz_out, runs)
    assert len(expect) == 3
    got_dev, got_host = files_of(dev_out), files_of(host_out)
    assert sorted(got_dev) == sorted(got_host) == sorted(expect)
    for f in expect:
        assert got_dev[f] == expect[f], (f, len(got_dev[f]), len(expect[f]))
        assert got_host[f] == expect[f], (f, len(got_host[f]), len(expect[f]))
    total = sum(len(r) for r in runs)
    c0, c1, c2, on_dev, on_host, gz = bins_of(dev.stderr)
    assert [c0, c1, c2] == count and c0 + c1 + c2 == n == len(dev.stdout.splitlines())
    assert on_host == tail and on_dev == total - tail and gz == int(gz_out)               # on the device route the host writes the tail alone
    c0, c1, c2, on_dev, on_host, gz = bins_of(host.stderr)
    assert [c0, c1, c2] == count and (on_dev, on_host, gz) == (0, total, int(gz_out))


def test_the_fallback_reads_the_file_again_and_leaves_the_same_files(work):
    d, n, want, _ = work
    for fmt, name, gz_out in (("fasta", "reads.fa", False), ("fastq", "reads.fq.gz", True)):
        rows, runs, count, tail = want[fmt]
        out = new_dir(d, "fallback_" + fmt)
        r = run(d, ["--read", name, "--format", fmt, "--ingest", "device", "--stats", "--bin-reads", "--bin-dir", str(out)] + (["--gz-out"] if gz_out else []),
                {"HAST_RS_BLOCK": "4096"})
        assert r.returncode == 0 and r.stdout == rows, r.stderr[-800:]
        assert r.stderr.count(b"WARN") == 1 and b"fallback=record_too_long" in r.stderr
        assert files_of(out) == expected_files("reads." + EXT[fmt][0], fmt, gz_out, runs)
        c0, c1, c2, on_dev, on_host, gz = bins_of(r.stderr)
        assert [c0, c1, c2] == count and on_dev == 0 and on_host == sum(len(x) for x in runs)


@pytest.mark.parametrize("ingest", ("device", "host"))
def test_a_format_error_leaves_no_files_of_its_input(work, ingest):
    d, n, want, _ = work
    for fmt in ("fasta", "fastq"):
        rows, runs, count, tail = want[fmt]
        ext = EXT[fmt][0]
        lines = (d / ("reads." + ext)).read_bytes().split(b"\n")
        at = len(lines) // 8 * 4 + (0 if fmt == "fastq" else 1)
        while fmt == "fasta" and (not lines[at] or lines[at][:1] == b">"):
            at += 1
        lines[at] = (b">" if fmt == "fastq" else b"@") + lines[at][1:]
        (d / ("bad." + ext)).write_bytes(b"\n".join(lines))
        out = new_dir(d, "bad_%s_%s" % (fmt, ingest))
        r = run(d, ["--read", "reads." + ext, "--read", "bad." + ext, "--format", fmt, "--ingest", ingest, "--bin-reads", "--bin-dir", str(out)],
                {"HAST_RS_BLOCK": "65536", "HAST_READ_BLOCK_BYTES": "65536"})
        assert r.returncode == 1 and r.stdout == rows and r.stderr.count(FORMAT_MSG[fmt]) == 1, r.stderr[-600:]
        assert files_of(out) == expected_files("reads." + ext, fmt, False, runs)          # the first input's, whole; none of the second's


def test_usage_errors_and_the_default_directory(work):
    d, n, want, _ = work
    before = sorted(os.listdir(d))
    (d / "sub").mkdir()
    (d / "sub" / "reads.fa.gz").write_bytes((d / "reads.fa.gz").read_bytes())
    for args in (["--read", "reads.fa", "--gz-out"], ["--read", "reads.fa", "--gz-out", "--ingest", "device"],
                 ["--read", "reads.fa", "--read", "sub/reads.fa.gz", "--bin-reads"], ["--read", "reads.fa", "--read", "./reads.fa", "--bin-reads", "--ingest", "device"]):
        r = run(d, args)
        assert r.returncode == 255 and r.stdout == b"" and b"__START__" not in r.stderr and b"--bin-reads" in r.stderr, args
    assert sorted(os.listdir(d)) == sorted(before + ["sub"])
    # without --bin-dir the files go to the working directory; a run without the flag writes none
    rows, runs, count, tail = want["fasta"]
    r = run(d, ["--read", "sub/reads.fa.gz", "--ingest", "device", "--bin-reads"], {"HAST_RS_BLOCK": "65536"})
    assert r.returncode == 0 and r.stdout == rows, r.stderr[-600:]
    made = sorted(set(os.listdir(d)) - set(before) - {"sub"})
    expect = expected_files("reads.fa", "fasta", False, runs)
    assert made == sorted(expect) and all((d / f).read_bytes() == expect[f] for f in made)
    for f in made:
        os.remove(d / f)
    r = run(d, ["--read", "reads.fa", "--ingest", "device"], {"HAST_RS_BLOCK": "65536"})
    assert r.returncode == 0 and r.stdout == rows and sorted(os.listdir(d)) == sorted(before + ["sub"])
    for ingest in ("device", "host"):                                        # a failed write: a message and exit 3
        r = run(d, ["--read", "reads.fa", "--ingest", ingest, "--bin-reads", "--bin-dir", "no/such/dir"], {"HAST_RS_BLOCK": "65536"})
        assert r.returncode == 3 and b"classify_read: ERROR: writing the reads of reads.fa" in r.stderr, (ingest, r.stderr[-400:])
