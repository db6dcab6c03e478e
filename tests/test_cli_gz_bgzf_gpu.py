"""classify --phase-reads --gz-out --gz-format bgzf (HAST_PHASE_GZ_FORMAT=bgzf): EVERY member of the routed <name>.<class>.fastq.gz files
is blocked gzip (BGZF) -- what the GPU deflates (dz_kernels.hip, k_dz_scan<true>) and what the host compresses (handed-over blocks,
tails, --route host, --host-parse: quartering.h bgzf_members) -- and every file ends with exactly one end-of-file block.  The
reference is THE SAME COMMAND WITHOUT THE FLAGS, as in tests/test_cli_gz_out_gpu.py (whose run_pair does the comparison): inflated
files, lists, filter_reads.log, stdout and stderr are the same.  A written file read back with --bgzf device is as many members as a
walk of the file counts, and prints what its plain bytes print."""
import gzip
import json
import os
import shutil
import subprocess

import pytest

import hast_amd
from tests.test_cli_gpu import _edge_fastq
from tests.test_cli_gz_out_gpu import run_pair
from tests.test_dz_blocked_cpu import EOF_BLOCK, walk_members
from tests.test_quartering_bgzf_cpu import check_bgzf_file

pytestmark = pytest.mark.gpu

BGZF = ("--gz-out", "--gz-format", "bgzf")
ARGS = ["--hap0", "hap0.mer", "--hap1", "hap1.mer", "--weight0", "1.04", "--read", "r1.fq", "--read", "r2.fq.gz", "--thread", "5", "--phase-reads"]


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(hast_amd.classify_exe()):
        hast_amd.build()
    return hast_amd.classify_exe()


def golden_dir(golden_workdir, d):
    shutil.copytree(golden_workdir / "rand_k21", d)
    with gzip.open(d / "r1.fq.gz") as f, open(d / "r1.fq", "wb") as g:
        shutil.copyfileobj(f, g)


def members_of_the_files(d, prefix=""):
    """every <prefix>*.fastq.gz of d is BGZF with one end-of-file block at its end; returns (members, bytes, inflated bytes) in all"""
    n = size = plain = 0
    for p in sorted(d.iterdir()):
        if p.name.startswith(prefix) and p.name.endswith(".fastq.gz"):
            z = p.read_bytes()
            b = gzip.decompress(z)
            n += check_bgzf_file(z, b)
            size += len(z)
            plain += len(b)
    return n, size, plain


@pytest.mark.parametrize("extra", [[], ["--route", "host"], ["--host-parse"], ["--devices", "0,0"], ["--devices", "0,0,0", "--batch-reads", "150"]])
def test_bgzf_in_the_configurations_of_the_phase_reads_test(exe, golden_workdir, tmp_path, extra):
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    for d in (a, b, c):
        golden_dir(golden_workdir, d)
    _, _, n_fastq = run_pair(exe, (a, b), ARGS, extra, gz_flag=BGZF)
    assert n_fastq >= 6
    assert members_of_the_files(b)[0] > n_fastq
    # --stats: format=bgzf (a gzip run's line says no format, as before), members counted as written (the end-of-file blocks among the host's)
    r = subprocess.run([exe] + ARGS + extra + list(BGZF) + ["--stats-json", "stats.json"], cwd=c, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-1000:]
    per_input = json.load(open(c / "stats.json"))["stats_route_gz"]
    assert [x["file"] for x in per_input] == ["r1.fq", "r2.fq.gz"] and all(x["format"] == "bgzf" for x in per_input)
    for x, prefix in zip(per_input, ("r1.fq.", "r2.fq.")):
        members, size, plain = members_of_the_files(c, prefix)
        assert x["device_members"] + x["host_members"] == members
        assert x["device_bytes_out"] + x["host_bytes_out"] == size
        assert x["device_bytes_in"] + x["host_bytes_in"] == plain
    if "--route" in extra or "--host-parse" in extra:
        assert all(x["device_members"] == 0 and x["host_members"] > 0 for x in per_input)
    else:
        assert sum(x["device_members"] for x in per_input) >= 6


@pytest.mark.parametrize("extra", [[], ["--batch-reads", "7"], ["--devices", "0,0,0", "--batch-reads", "16"]])
@pytest.mark.parametrize("tail", ["", "@t1#1_2_3/1\nACGTACGTACGTACGTACGTACGTACGT", "@t2#9_9_9/1\nACGTACGTACGTACGTACGTACGTACGT\n+\nFFFF"])
def test_bgzf_on_every_awk_branch(exe, golden_workdir, tmp_path, extra, tail):
    """the input of tests/test_cli_gz_out_gpu.py's awk-branch test: several blocks, blocks that come back to the host (a barcode of
    no list), ERROR lines, partial tails, plain and .gz: device-made and host-made BGZF members share the files"""
    recs = _edge_fastq()
    text = ("".join(recs) + tail).encode()
    dirs = (tmp_path / "plain", tmp_path / "packed")
    for d in dirs:
        shutil.copytree(golden_workdir / "rand_k21", d)
        (d / "e1.fq").write_bytes(text)
        with gzip.open(d / "e2.fq.gz", "wb") as g:
            g.write("".join(recs[:150]).encode() if not tail else text)
    args = ["--hap0", "hap0.mer", "--hap1", "hap1.mer", "--read", "e1.fq", "--read", "e2.fq.gz", "--thread", "3", "--phase-reads"]
    plain, packed, n_fastq = run_pair(exe, dirs, args, extra, gz_flag=BGZF)
    assert n_fastq >= 4
    assert len([l for l in packed.stderr.splitlines() if l.startswith(b"ERROR : unclassify")]) >= 20
    assert members_of_the_files(dirs[1])[0] >= 2 * n_fastq


def test_a_written_file_read_back_on_the_device_per_member(exe, golden_workdir, tmp_path):
    """--read <a file this program wrote> --bgzf device: __stats_bgzf__ counts the members a walk of the file counts, stdout is that of
    the file's plain bytes"""
    a, b = tmp_path / "a", tmp_path / "b"
    for d in (a, b):
        shutil.copytree(golden_workdir / "rand_k21", d)
    args = ["--hap0", "hap0.mer", "--hap1", "hap1.mer", "--read", "r1.fq.gz", "--phase-reads"]
    run_pair(exe, (a, b), args, [], gz_flag=BGZF)
    again = ["--hap0", "hap0.mer", "--hap1", "hap1.mer", "--stats", "--read"]
    p = subprocess.run([exe] + again + ["r1.fq.paternal.fastq"], cwd=a, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    z = subprocess.run([exe] + again + ["r1.fq.paternal.fastq.gz", "--bgzf", "device"], cwd=b, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0 and z.returncode == 0, z.stderr.decode()[-1000:]
    assert z.stdout == p.stdout and len(p.stdout) > 100
    lines = [l for l in z.stderr.decode().splitlines() if l.startswith("__stats_bgzf__")]
    assert len(lines) == 1, z.stderr.decode()[-1000:]
    fields = dict(kv.split("=", 1) for kv in lines[0].split()[1:])
    walked = walk_members((b / "r1.fq.paternal.fastq.gz").read_bytes())
    assert int(fields["members"]) == len(walked) > 2
    assert int(fields["inflated_bytes"]) == (a / "r1.fq.paternal.fastq").stat().st_size


def test_gzip_is_the_default_and_writes_the_bytes_of_gz_out_alone(exe, golden_workdir, tmp_path):
    dirs = {how: tmp_path / how for how in ("alone", "gzip", "env_ignored_by_the_flag")}
    got = {}
    for how, d in dirs.items():
        golden_dir(golden_workdir, d)
        flags = ["--gz-out"] + ([] if how == "alone" else ["--gz-format", "gzip"])
        env = dict(os.environ, HAST_PHASE_GZ_FORMAT="bgzf") if how == "env_ignored_by_the_flag" else None      # (the flag wins)
        r = subprocess.run([exe] + ARGS + flags, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert r.returncode == 0, r.stderr.decode()[-1000:]
        got[how] = {p.name: p.read_bytes() for p in d.iterdir() if p.name.endswith(".fastq.gz")}
    assert len(got["alone"]) >= 6 and got["alone"] == got["gzip"] == got["env_ignored_by_the_flag"]
    assert all(z[:4] == b"\x1f\x8b\x08\x00" and z[-28:] != EOF_BLOCK for z in got["alone"].values())
    r = subprocess.run([exe] + ARGS + ["--gz-out", "--gz-format", "gzip", "--stats"], cwd=dirs["gzip"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    lines = [l for l in r.stderr.decode().splitlines() if l.startswith("__stats_route_gz__")]
    assert r.returncode == 0 and len(lines) == 2 and not any("format=" in l for l in lines)


def test_the_environment_switch(exe, golden_workdir, tmp_path):
    """HAST_PHASE_GZ_FORMAT=bgzf beside HAST_PHASE_GZ=1 / --gz-out switches it on; without them it is ignored (plain files)"""
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    for d in (a, b, c):
        shutil.copytree(golden_workdir / "rand_k21", d)
    args = ["--hap0", "hap0.mer", "--hap1", "hap1.mer", "--read", "r1.fq.gz", "--thread", "3", "--phase-reads"]
    run_pair(exe, (a, b), args, [], env={"HAST_PHASE_GZ": "1", "HAST_PHASE_GZ_FORMAT": "bgzf"}, gz_flag=())
    assert members_of_the_files(b)[0] >= 6
    r = subprocess.run([exe] + args, cwd=c, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, HAST_PHASE_GZ_FORMAT="bgzf"))
    assert r.returncode == 0 and not any(p.name.endswith(".fastq.gz") for p in c.iterdir()) and any(p.name.endswith(".fastq") for p in c.iterdir())


@pytest.mark.parametrize("flags", [["--phase-reads", "--gz-format", "bgzf"], ["--phase-reads", "--gz-out", "--gz-format", "foo"], ["--gz-format", "bgzf"]])
def test_a_bad_use_is_the_usage_text_and_exit_255(exe, golden_workdir, tmp_path, flags):
    d = tmp_path / "w"
    shutil.copytree(golden_workdir / "rand_k21", d)
    before = sorted(p.name for p in d.iterdir())
    r = subprocess.run([exe, "--hap0", "hap0.mer", "--hap1", "no_such_file.mer", "--read", "r1.fq.gz"] + flags, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 255 and r.stdout == b""
    assert b"--gz-format" in r.stderr and b"classify --hap0" in r.stderr and b"no_such_file" not in r.stderr      # (before anything is read)
    assert sorted(p.name for p in d.iterdir()) == before
