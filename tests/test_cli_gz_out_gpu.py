"""classify --phase-reads --gz-out (HAST_PHASE_GZ=1): the routed files leave as <name>.<class>.fastq.gz -- records routed on the GPU are
deflated there (dz_kernels.hip) and only compressed bytes come back; what the host routes (handed-over blocks, tails, --route host) is
compressed by zlib as further members of the same files.  The reference for every case is THE SAME COMMAND WITHOUT THE FLAG, which
tests/test_cli_gpu.py pins to the wrapper's steps 10-11 and, through quartering_fastq, to the reference's awk program: gzip.decompress of
every .fastq.gz equals that command's plain file; the lists, filter_reads.log, stdout and stderr (but for the two time stamps) are the
same; no plain .fastq is left behind."""
import gzip
import json
import os
import re
import shutil
import subprocess
import zlib

import pytest

import hast_amd
from tests.conftest import GOLDEN
from tests.test_cli_gpu import _edge_fastq
from tests.test_dz_core_cpu import PIECE

pytestmark = pytest.mark.gpu

SUFFIXES = (".fastq", ".fastq.gz", ".barcodes", "filter_reads.log")
STAMP = re.compile(rb"^\w{3} \w{3} [ \d]\d \d\d:\d\d:\d\d \d{4}$")


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(hast_amd.classify_exe()):
        hast_amd.build()
    return hast_amd.classify_exe()


def stderr_lines(raw):
    return [l for l in raw.splitlines() if not STAMP.match(l)]


def run_pair(exe, dirs, args, extra, env=None, gz_flag=("--gz-out",)):
    """the command in dirs[0], the command with --gz-out in dirs[1]; returns both results and checks the files against each other"""
    plain = subprocess.run([exe] + args + extra, cwd=dirs[0], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert plain.returncode == 0, plain.stderr.decode()[-1500:]
    packed = subprocess.run([exe] + args + extra + list(gz_flag), cwd=dirs[1], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})))
    assert packed.returncode == 0, packed.stderr.decode()[-1500:]
    assert packed.stdout == plain.stdout
    assert stderr_lines(packed.stderr) == stderr_lines(plain.stderr)
    want = {p.name: p.read_bytes() for p in dirs[0].iterdir() if p.name.endswith(SUFFIXES)}
    got = {p.name: p.read_bytes() for p in dirs[1].iterdir() if p.name.endswith(SUFFIXES)}
    assert not any(n.endswith(".fastq") for n in got), sorted(got)
    assert not any(n.endswith(".fastq.gz") for n in want), sorted(want)
    assert sorted(n + ".gz" if n.endswith(".fastq") else n for n in want) == sorted(got)
    n_fastq = 0
    for name, data in want.items():
        if name.endswith(".fastq"):
            assert gzip.decompress(got[name + ".gz"]) == data, name
            n_fastq += 1
        else:
            assert got[name] == data, name
    for d in dirs:
        assert (d / "step_10_done").exists() and (d / "step_11_done").exists()
    return plain, packed, n_fastq


@pytest.mark.parametrize("extra", [[], ["--route", "host"], ["--devices", "0,0"], ["--devices", "0,0,0", "--batch-reads", "150"]])
def test_gz_out_in_the_configurations_of_the_phase_reads_test(exe, golden_workdir, tmp_path, extra):
    a, b = tmp_path / "a", tmp_path / "b"
    for d in (a, b):
        shutil.copytree(golden_workdir / "rand_k21", d)
        with gzip.open(d / "r1.fq.gz") as f, open(d / "r1.fq", "wb") as g:
            shutil.copyfileobj(f, g)
    args = ["--hap0", "hap0.mer", "--hap1", "hap1.mer", "--weight0", "1.04", "--read", "r1.fq", "--read", "r2.fq.gz", "--thread", "5", "--phase-reads"]
    _, _, n_fastq = run_pair(exe, (a, b), args, extra)
    assert n_fastq >= 6
    # --stats: what went into and came out of the encoders
    c = tmp_path / "c"
    shutil.copytree(golden_workdir / "rand_k21", c)
    with gzip.open(c / "r1.fq.gz") as f, open(c / "r1.fq", "wb") as g:
        shutil.copyfileobj(f, g)
    r = subprocess.run([exe] + args + extra + ["--gz-out", "--stats-json", "stats.json"], cwd=c, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-1000:]
    per_input = json.load(open(c / "stats.json"))["stats_route_gz"]        # one object per input, in the order of the inputs
    assert [x["file"] for x in per_input] == ["r1.fq", "r2.fq.gz"]
    for x, prefix in zip(per_input, ("r1.fq.", "r2.fq.")):
        files = [p for p in c.iterdir() if p.name.startswith(prefix) and p.name.endswith(".fastq.gz")]
        assert x["device_bytes_in"] + x["host_bytes_in"] == sum(len(gzip.decompress(p.read_bytes())) for p in files)
        assert x["device_bytes_out"] + x["host_bytes_out"] == sum(p.stat().st_size for p in files)
    st = {k: sum(x[k] for x in per_input) for k in per_input[0] if k != "file"}
    routed = sum(len(gzip.decompress(p.read_bytes())) for p in c.iterdir() if p.name.endswith(".fastq.gz"))
    written = sum(p.stat().st_size for p in c.iterdir() if p.name.endswith(".fastq.gz"))
    assert st["device_bytes_in"] + st["host_bytes_in"] == routed
    assert st["device_bytes_out"] + st["host_bytes_out"] == written
    if "--route" in extra:
        assert st["device_members"] == 0 and st["host_members"] > 0
    else:
        assert st["device_members"] >= 6 and st["device_bytes_out"] < st["device_bytes_in"]


def test_the_environment_switch(exe, golden_workdir, tmp_path):
    """HAST_PHASE_GZ=1 beside HAST_PHASE_READS / --phase-reads switches it on; alone it is ignored (a wrapper may export it for every stage)"""
    a, b = tmp_path / "a", tmp_path / "b"
    for d in (a, b):
        shutil.copytree(golden_workdir / "rand_k21", d)
    args = ["--hap0", "hap0.mer", "--hap1", "hap1.mer", "--read", "r1.fq.gz", "--thread", "3", "--phase-reads"]
    run_pair(exe, (a, b), args, [], env={"HAST_PHASE_GZ": "1"}, gz_flag=())
    c = tmp_path / "c"
    shutil.copytree(golden_workdir / "rand_k21", c)
    r = subprocess.run([exe] + args[:-1], cwd=c, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, HAST_PHASE_GZ="1"))
    assert r.returncode == 0 and not any(p.name.endswith((".fastq", ".fastq.gz")) for p in c.iterdir())


def test_the_flag_without_phase_reads_is_a_usage_error(exe, golden_workdir, tmp_path):
    d = tmp_path / "w"
    shutil.copytree(golden_workdir / "rand_k21", d)
    args = ["--hap0", "hap0.mer", "--hap1", "hap1.mer", "--read", "r1.fq.gz"]
    r = subprocess.run([exe] + args + ["--gz-out"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    bad = subprocess.run([exe] + args + ["--route", "nowhere"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0 and r.returncode == bad.returncode         # (as for the other flag errors)
    assert b"--gz-out" in r.stderr and b"classify --hap0" in r.stderr and r.stdout == b""
    assert not any(p.name.endswith((".fastq", ".fastq.gz")) for p in d.iterdir())


@pytest.mark.parametrize("extra", [[], ["--batch-reads", "7"], ["--devices", "0,0"], ["--devices", "0,0,0", "--batch-reads", "16"]])
@pytest.mark.parametrize("tail", ["", "@t1#1_2_3/1\nACGTACGTACGTACGTACGTACGTACGT", "@t2#9_9_9/1\nACGTACGTACGTACGTACGTACGTACGT\n+\nFFFF", "@t3#1_2_3/1"])
def test_gz_out_on_every_awk_branch(exe, golden_workdir, tmp_path, extra, tail):
    """the headers of tests/test_cli_gpu.py's awk-branch test (blocks that come back to the host, ERROR lines, dropped records) and its
    three kinds of partial tail, plain and .gz, small blocks, several contexts: device-made and zlib-made members share the files"""
    recs = _edge_fastq()
    text = ("".join(recs) + tail).encode()
    dirs = (tmp_path / "plain", tmp_path / "packed")
    for d in dirs:
        shutil.copytree(golden_workdir / "rand_k21", d)
        (d / "e1.fq").write_bytes(text)
        with gzip.open(d / "e2.fq.gz", "wb") as g:
            g.write("".join(recs[:150]).encode() if not tail else text)
    args = ["--hap0", "hap0.mer", "--hap1", "hap1.mer", "--read", "e1.fq", "--read", "e2.fq.gz", "--thread", "3", "--phase-reads"]
    plain, packed, n_fastq = run_pair(exe, dirs, args, extra)
    assert n_fastq >= 4
    assert len([l for l in packed.stderr.splitlines() if l.startswith(b"ERROR : unclassify")]) >= 20


def test_gz_out_on_the_quartering_goldens_edge_input(exe, golden_workdir, tmp_path):
    """the headers of the quartering goldens' hand-made edge input through `classify`.  Two things keep the golden outputs themselves
    out of reach of this program (they are checked byte for byte through the ABI in tests/test_dz_gpu.py and through the host tool in
    tests/test_quartering_gz_cpu.py): `classify` refuses reads shorter than K, as the reference does, and the edge input's reads are 1-4
    bases; and its lists come from its own calls, not from the golden lists.  So the base and quality lines are made 32 long (the
    partial last record's too) and the reference is the command without the flag: inflated outputs, filter_reads.log and the ERROR
    line on stderr byte for byte."""
    e = json.load(open(os.path.join(GOLDEN, "quartering", "expected.json")))["edge"]
    lines = e["inputs"]["e.fq"].split("\n")
    for i in range(len(lines)):
        if i % 4 == 1 and lines[i]:
            lines[i] = "ACGT" * 8
        elif i % 4 == 3 and lines[i]:
            lines[i] = "F" * 32
    text = "\n".join(lines)
    assert text.count("@r") == 9 and "@r8/5_5_5#z" in text and not text.endswith("F\n")
    dirs = (tmp_path / "plain", tmp_path / "packed")
    for d in dirs:
        shutil.copytree(golden_workdir / "rand_k21", d)
        (d / "e.fq").write_text(text)
    args = ["--hap0", "hap0.mer", "--hap1", "hap1.mer", "--read", "e.fq", "--phase-reads"]
    plain, packed, n_fastq = run_pair(exe, dirs, args, [])
    assert n_fastq >= 2
    errs = [l for l in packed.stderr.splitlines() if l.startswith(b"ERROR : unclassify")]
    assert errs == [l for l in plain.stderr.splitlines() if l.startswith(b"ERROR : unclassify")]
    assert errs == [b"ERROR : unclassify barcode : 5_5_5"]             # (@r8/5_5_5#z: awk looks "5_5_5" up, the list holds "z")
    assert (dirs[1] / "filter_reads.log").read_bytes() == (dirs[0] / "filter_reads.log").read_bytes()


def test_round_trip_a_routed_gz_file_as_read_input(exe, golden_workdir, tmp_path):
    """files this program writes are files it inflates on the GPU: `classify` on a routed paternal.fastq.gz (device inflate) prints what
    it prints on the plain file"""
    a, b = tmp_path / "a", tmp_path / "b"
    for d in (a, b):
        shutil.copytree(golden_workdir / "rand_k21", d)
    args = ["--hap0", "hap0.mer", "--hap1", "hap1.mer", "--read", "r1.fq.gz", "--phase-reads"]
    run_pair(exe, (a, b), args, [])
    again = ["--hap0", "hap0.mer", "--hap1", "hap1.mer", "--stats", "--read"]
    p = subprocess.run([exe] + again + ["r1.fq.paternal.fastq"], cwd=a, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    z = subprocess.run([exe] + again + ["r1.fq.paternal.fastq.gz"], cwd=b, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0 and z.returncode == 0, z.stderr.decode()[-1000:]
    assert z.stdout == p.stdout and len(p.stdout) > 100
    assert b"__stats_gz__" in z.stderr                       # (inflated on the device, not by the host decoders)


def test_gz_out_at_scale_with_the_default_block_size(exe, golden_workdir, tmp_path):
    """the production shape: the golden r1.fq tiled to 52 MB (record names repeat) in the default blocks of 16 MB, so a routed run is
    hundreds of 16-KB pieces and k_dz_scan (256 pieces a lap) goes round more than once.  The command without the flag is the
    reference, as above; and the members of every .fastq.gz are walked one by one: at least one member THE DEVICE made (its header
    says XFL = 0; zlib's level-1 members of handed-over blocks and tails say 4) inflates to more than 256 pieces."""
    tiles = 151
    with gzip.open(golden_workdir / "rand_k21" / "r1.fq.gz") as f:
        text = f.read() * tiles
    assert len(text) >= 50 << 20
    a, b = tmp_path / "a", tmp_path / "b"
    for d in (a, b):
        shutil.copytree(golden_workdir / "rand_k21", d)
        (d / "big.fq").write_bytes(text)
    args = ["--hap0", "hap0.mer", "--hap1", "hap1.mer", "--weight0", "1.04", "--read", "big.fq", "--thread", "5", "--phase-reads"]
    _, _, n_fastq = run_pair(exe, (a, b), args, [])
    assert n_fastq >= 3
    device_made, longest = 0, 0
    for p in sorted(b.iterdir()):
        if not p.name.endswith(".fastq.gz"):
            continue
        rest, sizes = p.read_bytes(), []
        while rest:
            d = zlib.decompressobj(31)
            n = len(d.decompress(rest))
            assert d.eof
            if rest[:10] == b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03":
                device_made += 1
                longest = max(longest, n)
            sizes.append(n)
            rest = d.unused_data
        print("%s: %d members, the longest inflates to %d bytes" % (p.name, len(sizes), max(sizes)))
    assert device_made > 0
    assert longest > 256 * PIECE, "no device-made member of more than 256 pieces: the longest inflates to %d bytes" % longest
