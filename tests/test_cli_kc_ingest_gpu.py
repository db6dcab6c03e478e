"""GPU test of `unshared_kmers --ingest device`: the parents' files inflated and framed on the GPU give the products the host
ingest gives; what the device path cannot take goes through the host parser after all, and the --stats line says which happened
(a silent fallback would pass every comparison of products)."""
import gzip
import os
import re
import shutil
import subprocess

import pytest

import hast_amd
from tests.conftest import golden_cases, load_case, run_s00_case

pytestmark = pytest.mark.gpu
EXE = hast_amd.unshared_kmers_exe()
DEVICE = ["--ingest", "device", "--stats"]


def ingest_line(stderr: bytes):
    m = re.search(rb"\[stats\] ingest device: blocks_framed=(\d+) gz_on_device=(\d+) fallback=(.*)", stderr)
    assert m, stderr[-1500:]
    return int(m.group(1)), int(m.group(2)), m.group(3).decode().strip()


def totals(stderr: bytes):
    rows = re.findall(rb"\[stats\] (paternal|maternal): (\d+) input bytes, (\d+) records, (\d+) bases, (\d+) k-mers counted", stderr)
    assert len(rows) == 2, stderr[-1500:]
    return rows


def on_device(res, gz):
    blocks, gz_dev, fallback = ingest_line(res.stderr)
    assert fallback == "none" and blocks > 0, res.stderr[-1500:]
    assert b"starting over with the host ingest" not in res.stderr
    if gz:
        assert gz_dev > 0
    return blocks


CASES = [(c, r) for c, r in golden_cases("s00") if c in ("s00_trio_k21", "s00_gz_k25")]


@pytest.mark.parametrize("case,run", CASES)
def test_device_ingest_matches_the_goldens(golden_workdir, tmp_path, case, run):
    res = run_s00_case(EXE, golden_workdir, tmp_path, case, run, extra_args=["--table-gb", "0.25"] + DEVICE)
    on_device(res, "gz" in case)


@pytest.mark.parametrize("case,run", CASES)
def test_device_ingest_in_small_blocks(golden_workdir, tmp_path, monkeypatch, case, run):
    monkeypatch.setenv("HAST_KC_INGEST_BLOCK", "4096")
    res = run_s00_case(EXE, golden_workdir, tmp_path, case, run, extra_args=["--table-gb", "0.25"] + DEVICE)
    assert on_device(res, "gz" in case) > 10            # (the inputs are tens of KB each)


@pytest.mark.parametrize("case,run", CASES)
def test_device_ingest_with_slices_and_a_table_that_overflows(golden_workdir, tmp_path, case, run):
    res = run_s00_case(EXE, golden_workdir, tmp_path, case, run, extra_args=["--table-gb", "0.00005", "--slices", "2"] + DEVICE)
    on_device(res, "gz" in case)
    assert b"count table full: starting over" in res.stderr


def test_flag_from_the_environment(golden_workdir, tmp_path, monkeypatch):
    monkeypatch.setenv("HAST_KC_INGEST", "device")
    res = run_s00_case(EXE, golden_workdir, tmp_path, "s00_trio_k21", "default_bounds", extra_args=["--table-gb", "0.25", "--stats"])
    on_device(res, False)


def test_gz_files_cut_inside_a_record_are_one_stream(golden_workdir, tmp_path):
    """the files of test_unshared_kmers_gz_files_cut_inside_a_record: the device feed reads a parent's .gz files in order and carries
    what one file leaves in front of the next, so there is nothing to start over for"""
    case, run = "s00_gz_k25", "gz"
    work = tmp_path / "recut"
    shutil.copytree(golden_workdir / case, work)
    for parent in "mp":
        # the script puts each new file in FRONT of the list: the stream is b then a
        whole = gzip.open(work / ("%s_b.fq.gz" % parent)).read() + gzip.open(work / ("%s_a.fq.gz" % parent)).read()
        cut = len(whole) // 3 + (17 if parent == "m" else 140)                 # inside a sequence / a quality line
        for name, part in (("b", whole[:cut]), ("a", whole[cut:])):
            with gzip.GzipFile(work / ("%s_%s.fq.gz" % (parent, name)), "wb", mtime=0) as f:
                f.write(part)
    meta = load_case(case)["runs"][run]
    res = subprocess.run([EXE] + meta["argv"] + ["--table-gb", "0.1"] + DEVICE, cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert res.returncode == 0, res.stderr[-1000:]
    on_device(res, True)
    assert b"in order" not in res.stderr
    for prod, rec in meta["products"].items():
        assert open(work / prod, "rb").read() == open(work / rec["expected"], "rb").read(), prod


@pytest.mark.parametrize("case,run,why", [("s00_edge_k31", "k31_auto", "four-line"), ("s00_edge_k31", "k32", "four-line"),
                                          ("s00_fasta_k11", "all", "FASTA"), ("s00_fasta_k11", "ge2", "FASTA")])
def test_what_the_framer_refuses_goes_through_the_host_parser(golden_workdir, tmp_path, case, run, why):
    res = run_s00_case(EXE, golden_workdir, tmp_path, case, run, extra_args=["--table-gb", "0.25"] + DEVICE)
    _, _, fallback = ingest_line(res.stderr)
    assert fallback != "none" and why in fallback, fallback
    assert b"starting over with the host ingest" in res.stderr and fallback.encode() in res.stderr.split(b"[stats]")[0]


def test_several_tables_use_the_host_ingest(golden_workdir, tmp_path):
    res = run_s00_case(EXE, golden_workdir, tmp_path, "s00_trio_k21", "default_bounds", extra_args=["--table-gb", "0.05", "--devices", "0,0"] + DEVICE)
    blocks, _, fallback = ingest_line(res.stderr)
    assert fallback == "several tables" and blocks == 0
    assert b"--ingest device works with one count table" in res.stderr


def test_input_errors_read_as_with_the_host_ingest(golden_workdir, tmp_path):
    work = tmp_path / "bad"
    shutil.copytree(golden_workdir / "s00_trio_k21", work)
    data = (work / "p2.fq").read_bytes()
    lines = data.split(b"\n")
    assert len(lines[3 + 4 * 50]) > 5
    lines[3 + 4 * 50] = lines[3 + 4 * 50][1:]           # one quality byte less in record 50
    (work / "p2.fq").write_bytes(b"\n".join(lines))
    argv = load_case("s00_trio_k21")["runs"]["default_bounds"]["argv"] + ["--table-gb", "0.05"]
    runs = [subprocess.run([EXE] + argv + ["--ingest", how], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE) for how in ("host", "device")]
    errors = [[l for l in r.stdout.splitlines() if l.startswith(b"ERROR:")] for r in runs]
    assert runs[0].returncode == runs[1].returncode == 1 and errors[0] == errors[1] and len(errors[0]) == 1, (errors, runs[1].stderr[-500:])
    assert b"starting over with the host ingest" in runs[1].stderr


@pytest.mark.parametrize("case,run", [("s00_trio_k21", "default_bounds"), ("s00_gz_k25", "gz")])
def test_totals_equal_the_host_ingests(golden_workdir, tmp_path, case, run):
    host = run_s00_case(EXE, golden_workdir, tmp_path / "h", case, run, extra_args=["--table-gb", "0.25", "--ingest", "host", "--stats"])
    dev = run_s00_case(EXE, golden_workdir, tmp_path / "d", case, run, extra_args=["--table-gb", "0.25"] + DEVICE)
    on_device(dev, "gz" in case)
    assert b"ingest device" not in host.stderr
    assert totals(host.stderr) == totals(dev.stderr)


def test_bad_value_of_the_flag(golden_workdir):
    d = golden_workdir / "s00_trio_k21"
    r = subprocess.run([EXE, "--paternal", "p1.fq", "--maternal", "m.fq", "--ingest", "gpu"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"--ingest" in r.stdout
