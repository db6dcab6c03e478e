"""`classify --rows device` (HAST_ROWS): the output table, and with --phase-reads the three barcode lists, keyed, called, sorted and
formatted on the GPU (hast_rows_*).  The bytes are the reference's on every golden case, with one and with several contexts; every
run the device cannot do this for goes the host's way with its reason and the same bytes; --phase-reads leaves the same files as
--rows host, also with a table of several tiles of barcodes; the flag's alias, its usage error, a full disk, and no word of it in the stats of a run that did not ask."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import hast_amd
from tests.conftest import golden_cases, load_case

pytestmark = pytest.mark.gpu

RAND = ["--hap0", "hap0.mer", "--hap1", "hap1.mer", "--weight0", "1.04", "--read", "r1.fq.gz", "--read", "r2.fq.gz", "--thread", "5"]


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(hast_amd.classify_exe()):
        hast_amd.build()
    return hast_amd.classify_exe()


def run(exe, args, cwd, env=None, **kw):
    clean = {k: v for k, v in os.environ.items() if k != "HAST_ROWS"}
    return subprocess.run([exe] + args, cwd=cwd, stdout=kw.pop("stdout", subprocess.PIPE), stderr=subprocess.PIPE, env=dict(clean, **(env or {})), timeout=600, **kw)


def rows_line(res):
    """the key=value pairs of the run's __stats_rows__ line; None when there is none"""
    lines = [l for l in res.stderr.decode().splitlines() if l.startswith("__stats_rows__")]
    assert len(lines) <= 1
    return dict(x.split("=", 1) for x in lines[0].split()[1:]) if lines else None


@pytest.fixture(scope="module")
def rand_ref(exe, golden_workdir):
    """rand_k21 without the flag: the bytes every route has to print"""
    r = run(exe, RAND, golden_workdir / "rand_k21")
    assert r.returncode == 0, r.stderr.decode()[-1000:]
    return r.stdout


@pytest.mark.parametrize("extra", [[], ["--devices", "0,0"]], ids=["one_context", "devices_0_0"])
@pytest.mark.parametrize("case,run_name", golden_cases("s01"))
def test_rows_device_prints_the_references_bytes(exe, golden_workdir, case, run_name, extra):
    meta = load_case(case)["runs"][run_name]
    d = golden_workdir / case
    r = run(exe, meta["argv"] + ["--rows", "device", "--stats"] + extra, d)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    want = open(d / meta["expected"], "rb").read()
    assert r.stdout == want
    kv = rows_line(r)
    assert kv and kv["route"] == "device" and kv["fallback"] == "none", kv
    assert int(kv["rows"]) == want.count(b"\n") and int(kv["table_bytes"]) == len(want), kv
    assert b"WARN : --rows device" not in r.stderr


def dictionary_line(res):
    line = [l for l in res.stderr.decode().splitlines() if l.startswith("__stats_dictionary__")][0]
    return dict(x.split("=", 1) for x in line.split()[1:])


@pytest.mark.parametrize("env,extra,reason", [({"HAST_NAME_DICT": "0"}, [], "no_device_dictionary"), ({"HAST_NAME_CACHE": "16"}, [], "host_names"),
                                              ({"HAST_NAME_DICT": "context"}, ["--devices", "0,0,0"], "several_dictionaries")])
def test_every_fallback_prints_the_same_bytes_and_says_why(exe, golden_workdir, rand_ref, env, extra, reason):
    """(host_names: a dictionary asked to hold 16 barcodes hands out 32 ids, rand_k21 has 60 barcodes: the host names the rest)"""
    r = run(exe, RAND + ["--rows", "device", "--stats"] + extra, golden_workdir / "rand_k21", env=env)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == rand_ref
    kv = rows_line(r)
    assert kv and kv["route"] == "host" and kv["fallback"] == reason, kv
    warn = [l for l in r.stderr.decode().splitlines() if "WARN : --rows device" in l]
    assert len(warn) == 1 and ("fallback=" + reason) in warn[0]
    if reason == "host_names":
        assert int(dictionary_line(r)["ids_from_host"]) > 0


def test_a_dictionary_of_64_ids_falls_back_exactly_when_the_host_named_a_barcode(exe, golden_workdir, rand_ref):
    """HAST_NAME_CACHE=64 on rand_k21: the same stdout; the reason is host_names if the host named a barcode and the route is the
    device's if it named none.  (rand_k21 has 60 barcodes, which 64 ids hold: with this input the device route is taken; the test
    above makes the dictionary too small for it.)"""
    r = run(exe, RAND + ["--rows", "device", "--stats"], golden_workdir / "rand_k21", env={"HAST_NAME_CACHE": "64"})
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == rand_ref
    kv, named_by_host = rows_line(r), int(dictionary_line(r)["ids_from_host"])
    if named_by_host or rand_ref.count(b"\n") > 64:
        assert (kv["route"], kv["fallback"]) == ("host", "host_names"), kv
    else:
        assert (kv["route"], kv["fallback"]) == ("device", "none"), kv


def test_counters_read_back_on_the_way_are_a_fallback(exe, golden_workdir, rand_ref):
    """counters sized for 3 barcodes grow during the read phase: what was counted so far is folded into the host's sums"""
    r = run(exe, RAND + ["--rows", "device", "--stats", "--initial-barcodes", "3", "--batch-reads", "97"], golden_workdir / "rand_k21")
    assert r.returncode == 0 and r.stdout == rand_ref, r.stderr.decode()[-2000:]
    kv = rows_line(r)
    assert kv["route"] == "host" and kv["fallback"] == "counts_on_host", kv


def test_the_alias_the_flag_and_a_run_that_did_not_ask(exe, golden_workdir, rand_ref):
    d = golden_workdir / "rand_k21"
    r = run(exe, RAND + ["--stats"], d, env={"HAST_ROWS": "device"})
    assert r.returncode == 0 and r.stdout == rand_ref and rows_line(r)["route"] == "device"
    r = run(exe, RAND + ["--stats", "--rows", "host"], d, env={"HAST_ROWS": "device"})          # the flag wins
    assert r.returncode == 0 and r.stdout == rand_ref and rows_line(r) is None
    r = run(exe, RAND + ["--stats"], d)
    assert r.returncode == 0 and r.stdout == rand_ref and b"__stats_rows__" not in r.stderr
    js = d / "rows_stats.json"
    r = run(exe, RAND + ["--rows", "device", "--stats-json", str(js)], d)
    assert r.returncode == 0 and r.stdout == rand_ref
    import json
    rows = json.load(open(js))["stats_rows"]
    assert rows["route"] == "device" and rows["fallback"] == "none" and rows["table_bytes"] == len(rand_ref) and rows["list_bytes"] == "0,0,0"
    os.remove(js)


def test_a_wrong_value_is_the_usage_text_before_anything_is_read(exe, tmp_path):
    for args, env in ((["--rows", "foo"], {}), ([], {"HAST_ROWS": "gpu"})):
        r = run(exe, ["--hap0", "no_such_file", "--hap1", "no_such_file", "--read", "no_such_file"] + args, tmp_path, env=env)
        assert r.returncode == 255 and b"--rows MODE" in r.stderr and b"__START__" not in r.stderr and r.stdout == b""


def test_a_full_disk_is_not_exit_0(exe, golden_workdir):
    with open("/dev/full", "wb") as full:
        r = run(exe, RAND + ["--rows", "device"], golden_workdir / "rand_k21", stdout=full)
    assert r.returncode == 2 and b"writing the result to stdout failed" in r.stderr, r.stderr[-300:]


def edge_fastq(seed=5, long_barcodes=True, sep=False):
    """the records of test_cli_gpu.py's awk-branch test, built here: headers that take every branch of quartering_fastq.awk:21-49"""
    rng = np.random.default_rng(seed)

    def seq(n=60):
        return "".join("ACGT"[i] for i in rng.integers(0, 4, n))
    heads = ["@a1#1_2_3/1", "@a2#0_0_0/1", "@a3", "@a4/x#5_6_7/1", "@a5#averyveryverylongbarcode_123/1", "@a6#1_2_3", "@a7#/1", "@a8#7_8_9/2\t5\t1",
             "@a9#1_2_3/1", "@b1/1", "@b2#0_0/1", "@b3#0/1", "@b4#exactly15bytes_/1", "@b5#sixteen_bytes_xx/1", "@b6#4_4_4#5_5_5/1", "@b7#0_0_0"]
    if not long_barcodes:
        heads = [h for h in heads if not h.startswith(("@a5", "@b5"))]
    recs = ["%s\n%s\n+\n%s\n" % (heads[i % len(heads)], seq(), "F" * 60) for i in range(400)]
    if sep:
        recs.append("@c1#1_2_3/1/2\n" + "ACGT" * 15 + "\n+\n" + "F" * 60 + "\n")
    return recs


def phase_reads_files(exe, src, tmp_path, reads, mode, make_inputs):
    d = tmp_path / mode
    shutil.copytree(src, d)
    make_inputs(d)
    args = ["--hap0", "hap0.mer", "--hap1", "hap1.mer", "--weight0", "1.04", "--thread", "3", "--stats", "--phase-reads", "--rows", mode]
    for x in reads:
        args += ["--read", x]
    r = run(exe, args, d)
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    err = [l for l in r.stderr.decode().splitlines() if l.startswith("ERROR : unclassify")]
    files = {p.name: p.read_bytes() for p in d.iterdir() if p.name.endswith((".fastq", ".barcodes", "filter_reads.log"))}
    markers = sorted(p.name for p in d.iterdir() if p.name.startswith("step_"))
    route = [l for l in r.stderr.decode().splitlines() if l.startswith("__stats_phase_reads__")][0]
    return r.stdout, err, files, markers, rows_line(r), route


MANY_TILES = 5                                      # many_barcodes: more rows than this many tiles of 512 (rows::kTile)


def many_barcodes_fastq(d):
    """rand_k21's reads under other headers: nearly every record a barcode of its own, of at most 15 bytes, in no order of the texts --
    some 2800 rows, six tiles of k_rows_write; every tenth record of the second file shares its mate's barcode, every 97th has 0_0_0"""
    out = []
    for k, name in enumerate(("r1.fq.gz", "r2.fq.gz")):
        with gzip.open(d / name, "rb") as f:
            lines = f.read().split(b"\n")
        recs = []
        for i in range(len(lines) // 4):
            j = i if k == 0 or i % 10 == 3 else 1500 + i
            code = b"0_0_0" if i % 97 == 5 else b"%d_%d_%d" % (1 + j * 7 % 1536, 1 + j * 11 % 1536, 1 + j)
            assert len(code) <= 15
            recs.append(b"@M%d#%s/%d\n" % (i, code, k + 1) + b"\n".join(lines[4 * i + 1:4 * i + 4]) + b"\n")
        out.append(b"".join(recs))
    assert len({r.split(b"#")[1].split(b"/")[0] for o in out for r in o.split(b"\n")[0::4] if r}) > MANY_TILES * 512
    return out


JOBS = {
    # name: (inputs, the route of the table with --rows device, its reason, the router)
    "rand_k21": (None, "device", "none", "route=device"),
    "edge": (dict(), "host", "host_names", "route=device"),                          # (barcodes of 16 bytes and more are the host's to name)
    "edge_short": (dict(long_barcodes=False), "device", "none", "route=device"),
    "edge_with_separator": (dict(long_barcodes=False, sep=True), "device", "none", "route=host"),
    "many_barcodes": ("many", "device", "none", "route=device"),                     # (the table has a second tile, and a sixth)
}


@pytest.mark.parametrize("job", sorted(JOBS))
def test_phase_reads_leaves_the_same_files_as_rows_host(exe, golden_workdir, tmp_path, job):
    edge, route, reason, router = JOBS[job]

    def make_inputs(d):
        if edge is None:
            return
        if edge == "many":
            one, two = many_barcodes_fastq(d)
            (d / "e1.fq").write_bytes(one)
            with gzip.open(d / "e2.fq.gz", "wb") as g:
                g.write(two)
            return
        recs = edge_fastq(**edge)
        (d / "e1.fq").write_bytes("".join(recs).encode())
        with gzip.open(d / "e2.fq.gz", "wb") as g:
            g.write("".join(recs[:150]).encode())
    reads = ["r1.fq.gz", "r2.fq.gz"] if edge is None else ["e1.fq", "e2.fq.gz"]
    dev = phase_reads_files(exe, golden_workdir / "rand_k21", tmp_path, reads, "device", make_inputs)
    host = phase_reads_files(exe, golden_workdir / "rand_k21", tmp_path, reads, "host", make_inputs)
    assert dev[0] == host[0] and dev[1] == host[1] and dev[3] == host[3] == ["step_10_done", "step_11_done"]
    assert sorted(dev[2]) == sorted(host[2]) and len([n for n in host[2] if n.endswith(".barcodes")]) == 3
    for name, data in host[2].items():
        assert dev[2][name] == data, name
    assert host[4] is None and dev[4]["route"] == route and dev[4]["fallback"] == reason, dev[4]
    assert router in dev[5] and router in host[5], (dev[5], host[5])
    if route == "device":
        sizes = [len(host[2][n + ".unique.barcodes"]) for n in ("paternal", "maternal", "homozygous")]
        assert dev[4]["list_bytes"] == "%d,%d,%d" % tuple(sizes) and int(dev[4]["table_bytes"]) == len(host[0])
    if job == "many_barcodes":
        assert int(dev[4]["rows"]) > MANY_TILES * 512 and int(dev[4]["rows"]) == host[0].count(b"\n"), dev[4]
