"""`classify --bgzf device` (HAST_BGZF=device): blocked-gzip inputs inflated on the GPU per member (hast_gz_open_blocked) instead of on
host threads.  The golden case's two .fq.gz inputs are re-blocked here; the run must print what the reference printed, route the
same reads with --phase-reads (device and host router), say so in --stats, stay on the host without the flag and in a striped run,
and end with exit 2 and the file's name on a damaged input."""
import gzip
import os
import shutil
import subprocess

import pytest

import hast_amd
from tests.conftest import load_case
from tests.test_inflate_cpu import bgzf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(hast_amd.classify_exe()):
        hast_amd.build()
    return hast_amd.classify_exe()


@pytest.fixture()
def case_dir(golden_workdir, tmp_path):
    d = tmp_path / "bgzf"
    shutil.copytree(golden_workdir / "rand_k21", d)
    for name in ("r1.fq.gz", "r2.fq.gz"):
        (d / name).write_bytes(bgzf(gzip.decompress((d / name).read_bytes())))
    return d


def run(exe, d, args, env=None):
    e = dict(os.environ)
    e.pop("HAST_BGZF", None)
    e.update(env or {})
    return subprocess.run([exe] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=600)


def stat_lines(r):
    return [l for l in r.stderr.decode().splitlines() if l.startswith("__stats_bgzf__")]


def test_cli_bgzf_device_prints_the_golden_output(exe, case_dir):
    meta = load_case("rand_k21")["runs"]["pair_w104"]
    want = open(case_dir / meta["expected"], "rb").read()
    for extra, env in ((["--bgzf", "device"], None), ([], {"HAST_BGZF": "device"}), (["--bgzf", "device", "--block-mb", "1"], None),
                       (["--bgzf", "device", "--batch-reads", "13"], {"HAST_BZ_BATCH_IN_BYTES": "70000", "HAST_BZ_BATCH_OUT_BYTES": "65536"})):
        r = run(exe, case_dir, meta["argv"] + ["--stats"] + extra, env)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert r.stdout == want, (extra, env)
        lines = stat_lines(r)
        assert len(lines) == 2, r.stderr.decode()[-2000:]
        for l in lines:
            kv = dict(x.split("=", 1) for x in l.split()[1:])
            assert int(kv["members"]) > 0 and int(kv["batches"]) > 0 and {"file", "read_s", "upload_s", "kernels_s"} <= set(kv), l
        assert b"__stats_gz__" not in r.stderr


def test_cli_bgzf_stays_on_the_host_unless_asked(exe, case_dir):
    """without the flag, with --bgzf host (the flag wins over the variable) and in a striped run: the host route, the same output"""
    meta = load_case("rand_k21")["runs"]["pair_w104"]
    want = open(case_dir / meta["expected"], "rb").read()
    for extra, env in (([], None), (["--bgzf", "host"], {"HAST_BGZF": "device"}), (["--devices", "0,0", "--bgzf", "device"], None)):
        r = run(exe, case_dir, meta["argv"] + ["--stats"] + extra, env)
        assert r.returncode == 0 and r.stdout == want, (extra, r.stderr.decode()[-1000:])
        assert stat_lines(r) == [] and b"__stats_gz__" not in r.stderr, extra
    # whole files dealt to two contexts: each file inflated on its context's GPU
    r = run(exe, case_dir, meta["argv"] + ["--stats", "--devices", "0,0", "--deal", "files", "--bgzf", "device"])
    assert r.returncode == 0 and r.stdout == want and len(stat_lines(r)) == 2, r.stderr.decode()[-1000:]


def test_cli_bgzf_stats_json(exe, case_dir, tmp_path):
    meta = load_case("rand_k21")["runs"]["pair_w104"]
    js = tmp_path / "stats.json"
    r = run(exe, case_dir, meta["argv"] + ["--bgzf", "device", "--stats-json", str(js)])
    assert r.returncode == 0, r.stderr.decode()[-1000:]
    import json
    bz = json.load(open(js))["stats_bgzf"]
    assert isinstance(bz, list) and len(bz) == 2
    assert all(b["members"] > 0 and b["batches"] > 0 and b["inflated_bytes"] > b["compressed_bytes"] > 0 and b["kernels_s"] >= 0 for b in bz)


@pytest.mark.parametrize("route", [[], ["--route", "host"]])
def test_cli_bgzf_phase_reads_routes_the_same_reads(exe, case_dir, tmp_path, route):
    meta = load_case("rand_k21")["runs"]["pair_w104"]
    made = {}
    for mode in ("host", "device"):
        d = tmp_path / ("run_" + mode)
        shutil.copytree(case_dir, d)
        r = run(exe, d, meta["argv"] + ["--phase-reads", "--stats", "--bgzf", mode] + route)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        assert len(stat_lines(r)) == (2 if mode == "device" else 0)
        made[mode] = (r.stdout, {p.name: p.read_bytes() for p in d.iterdir() if p.name.endswith((".fastq", ".barcodes", "filter_reads.log"))})
    assert made["device"][0] == made["host"][0] == open(case_dir / meta["expected"], "rb").read()
    files = made["host"][1]
    assert sum(1 for n in files if n.endswith(".fastq")) >= 4 and "filter_reads.log" in files and sum(1 for n in files if n.endswith(".barcodes")) == 3, sorted(files)
    assert made["device"][1] == files


def test_cli_bgzf_usage_and_damage(exe, case_dir):
    meta = load_case("rand_k21")["runs"]["pair_w104"]
    r = run(exe, case_dir, meta["argv"] + ["--bgzf", "sideways"])
    assert r.returncode == 255 and r.stdout == b""
    r = run(exe, case_dir, meta["argv"], {"HAST_BGZF": "sideways"})
    assert r.returncode == 255 and r.stdout == b""
    whole = (case_dir / "r2.fq.gz").read_bytes()
    flipped = bytearray(whole)
    flipped[len(whole) // 3] ^= 0x10
    for damaged in (bytes(flipped), whole[:len(whole) // 2]):
        (case_dir / "r2.fq.gz").write_bytes(damaged)
        r = run(exe, case_dir, meta["argv"] + ["--bgzf", "device"])
        assert r.returncode == 2 and r.stdout == b"", r.stderr.decode()[-500:]
        assert b"r2.fq.gz" in r.stderr and b"--bgzf host" in r.stderr and b"offset" in r.stderr, r.stderr.decode()[-500:]
    # an ordinary gzip member in mid-file: the same end, with the offset
    (case_dir / "r2.fq.gz").write_bytes(whole + gzip.compress(b"@x#1_1_1/1\nACGT\n+\nFFFF\n"))
    r = run(exe, case_dir, meta["argv"] + ["--bgzf", "device"])
    assert r.returncode == 2 and b"r2.fq.gz" in r.stderr and str(len(whole)).encode() in r.stderr and b"--bgzf host" in r.stderr, r.stderr.decode()[-500:]
