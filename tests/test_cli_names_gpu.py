"""The barcode dictionary at and past its last id, through the command line (-m gpu).  The device dictionary holds --name-cache ids
(16M by default; stLFR libraries carry more); once they are out the host numbers what arrives, in a range of its own, and the output
has one row per id.  Every case here RUNS OUT -- __stats_dictionary__ must say so -- and must still print what the reference prints:
no barcode on two rows with its counts split, no exit 4 after the whole read phase (several dictionaries, the first one full at a
merge).  The rows of test_cli_who_numbers_the_barcodes with HAST_NAME_CACHE=64 never got there: 64 ids against 60 barcodes.
The program of round 10 on these cases, once, on an MI355X: of the 28 golden runs 7 ended with exit 4 (a dictionary per context, small
blocks or whole files dealt) and 1 printed two barcodes twice (rand_k21 wrapper_argv, two contexts sharing the dictionary); of the 7
generated runs 2 ended with exit 4 and 4 printed 9 to 29 barcodes twice -- also the plain one, one context, no flag but --name-cache."""
import gzip
import os
import shutil
import subprocess

import pytest

import hast_amd
from tests.conftest import ROOT, golden_cases, load_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(hast_amd.classify_exe()):
        hast_amd.build()
    return hast_amd.classify_exe()


def stats_of(stderr, section):
    line = [l for l in stderr.decode().splitlines() if l.startswith("__stats_%s__" % section)]
    assert len(line) == 1, stderr.decode()[-2000:]
    return dict(x.split("=", 1) for x in line[0].split()[1:] if "=" in x)


def no_barcode_twice(stdout):
    names = [r.split(b"\t")[0] for r in stdout.splitlines()]
    assert len(names) == len(set(names)), [n for n in set(names) if names.count(n) > 1][:5]


# HAST_NAME_CACHE=16: the smallest dictionary there is -- 64 slots, 32 ids -- against 60 (rand_k21) and 40 (rand_k11) barcodes
RUNS_OUT = [
    ("one", {}, []),
    ("one_small_blocks", {}, ["--batch-reads", "97", "--initial-barcodes", "3"]),
    ("shared", {}, ["--devices", "0,0"]),
    ("shared_small_blocks", {}, ["--devices", "0,0", "--batch-reads", "50", "--initial-barcodes", "7"]),
    ("per_context", {"HAST_NAME_DICT": "context"}, ["--devices", "0,0"]),
    ("per_context_small_blocks", {"HAST_NAME_DICT": "context"}, ["--devices", "0,0", "--batch-reads", "50", "--initial-barcodes", "7"]),
    ("per_context_files", {"HAST_NAME_DICT": "context", "HAST_DEAL": "files"}, ["--devices", "0,0,0"]),
]


@pytest.mark.parametrize("name,env,extra", RUNS_OUT, ids=[r[0] for r in RUNS_OUT])
@pytest.mark.parametrize("case,run", [cr for cr in golden_cases("s01") if cr[0] in ("rand_k21", "rand_k11")])
def test_cli_dictionary_runs_out(exe, golden_workdir, case, run, name, env, extra):
    """one dictionary; one with blocks of 97 records and counters that regrow under both numberings; one shared by two contexts
    (their kernels claim in it at the same time); one per context, merged by text into the first, which is full; one per context with
    whole files dealt, so that they fill at different rates and each hands to the host what the other has numbered"""
    meta = load_case(case)["runs"][run]
    d = golden_workdir / case
    res = subprocess.run([exe] + meta["argv"] + extra + ["--stats"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600,
                         env=dict(os.environ, HAST_NAME_CACHE="16", **env))
    assert res.returncode == 0, (res.returncode, res.stderr.decode()[-2000:])
    want = open(d / meta["expected"], "rb").read()
    kv = stats_of(res.stderr, "dictionary")
    print(case, run, name, kv)
    no_barcode_twice(res.stdout)
    assert res.stdout == want
    assert len(want.splitlines()) > 32                           # the case has more barcodes than the dictionary has ids
    assert int(kv["ids_limit"]) == 32 and int(kv["ids_from_device"]) == 32, kv
    assert int(kv["ids_from_host"]) > 0, kv
    assert int(kv["dictionaries"]) == (len(extra[extra.index("--devices") + 1].split(",")) if "HAST_NAME_DICT" in env else 1), kv


def test_cli_200k_barcodes_through_a_dictionary_of_65536(exe, oracle_dir, tmp_path):
    """300 000 read pairs over 200 000 barcodes (some 155 000 of them seen) through --name-cache 65536: the blocks in which the last
    ids go hold tens of thousands of records, in hundreds of workgroups, with the occurrences of a barcode spread over them.  One
    context, two that share the dictionary, three with one each (merged by text into the first, which is full long before), r2 as
    .gz.  stdout == the oracle's restatement of classify.cpp, byte for byte; no barcode on two rows."""
    gen = os.path.join(ROOT, "tools", "gen_fastq")
    if not os.path.exists(gen):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools"), "gen_fastq"], check=True)
    d = tmp_path / "c"
    d.mkdir()
    try:
        subprocess.run([gen, str(d), "300000", "200000", "200000", "21", "150", "8"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        with open(d / "r2.fq", "rb") as f, gzip.open(d / "r2.fq.gz", "wb", compresslevel=1) as g:
            shutil.copyfileobj(f, g, 1 << 24)
        args = ["--hap0", "hap0.mer", "--hap1", "hap1.mer", "--thread", "16", "--weight0", "1.04", "--read", "r1.fq"]
        ref = subprocess.run([os.path.join(oracle_dir, "oracle_classify")] + args + ["--read", "r2.fq"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
        assert ref.returncode == 0, ref.stderr.decode()[-500:]
        n_rows = len(ref.stdout.splitlines())
        assert 140_000 < n_rows < 170_000                         # 200k x (1 - exp(-1.5)): far more than 65536
        no_barcode_twice(ref.stdout)
        for env, extra in (({}, ["--read", "r2.fq"]), ({}, ["--read", "r2.fq", "--devices", "0,0"]), ({}, ["--read", "r2.fq", "--devices", "0,0", "--batch-reads", "20000"]),
                           ({"HAST_NAME_DICT": "context"}, ["--read", "r2.fq", "--devices", "0,0,0"]),
                           ({"HAST_NAME_DICT": "context", "HAST_DEAL": "files"}, ["--read", "r2.fq", "--devices", "0,0"]),
                           ({}, ["--read", "r2.fq.gz"]), ({}, ["--read", "r2.fq.gz", "--devices", "0,0"])):
            got = subprocess.run([exe] + args + extra + ["--name-cache", "65536", "--stats"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900,
                                 env=dict(os.environ, **env))
            assert got.returncode == 0, (env, extra, got.returncode, got.stderr.decode()[-2000:])
            kv = stats_of(got.stderr, "dictionary")
            print(env, extra, kv)
            no_barcode_twice(got.stdout)
            assert got.stdout == ref.stdout, (env, extra, len(got.stdout.splitlines()), n_rows)
            assert int(kv["ids_limit"]) == 65536 and int(kv["ids_from_device"]) == 65536 and int(kv["ids_from_host"]) > 0, kv
    finally:
        shutil.rmtree(d, ignore_errors=True)


def test_cli_sizes_with_suffixes_mean_what_they_say(exe, golden_workdir):
    """--name-cache 16M is the usage text's own spelling of the default: atol made a dictionary of 16 out of it (32 ids).  K, M and G are
    powers of 1024; --park-gb takes a decimal number."""
    meta = load_case("rand_k21")["runs"]["pair_w104"]
    d = golden_workdir / "rand_k21"
    want = open(d / meta["expected"], "rb").read()
    for flags, sizes, limit in ((["--name-cache", "16M"], {"name_cache": str(16 << 20)}, 16 << 20),
                                (["--name-cache", "65536"], {"name_cache": "65536"}, 65536),
                                (["--name-cache", "64K", "--gz-ring-bytes", "2G", "--park-gb", "1.5"],
                                 {"name_cache": "65536", "gz_ring_bytes": str(2 << 30), "park_gb": "1.5"}, 65536),
                                (["--name-cache", "1k", "--gz-ring-bytes", "4096"], {"name_cache": "1024", "gz_ring_bytes": "4096"}, 1024)):
        res = subprocess.run([exe] + meta["argv"] + flags + ["--stats"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert res.returncode == 0, (flags, res.stderr.decode()[-2000:])
        assert res.stdout == want, flags
        got = stats_of(res.stderr, "sizes")
        for key, val in sizes.items():
            assert got[key] == val, (flags, got)
        kv = stats_of(res.stderr, "dictionary")
        assert int(kv["ids_limit"]) == limit and int(kv["ids_from_host"]) == 0, (flags, kv)
