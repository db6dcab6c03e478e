"""GPU test of `unshared_kmers --ingest device --device-fasta`: FASTA parents framed on the GPU give the products, totals, messages and
exit statuses the host ingest gives, and the two --stats lines say that the device route ran (a silent fallback would pass every
comparison of products).

The files of tests/golden/s00_fasta_k11 hold lines of up to 303 bytes, so at HAST_KC_INGEST_BLOCK=64 they are the case "a line
longer than a block" (asserted below: the "full block" fallback, and still the goldens); the small-block runs that must stay on the
device use the same records folded to 7 columns at 64 bytes a block, and the files as they are at 512 (more than 10 blocks) and 4096."""
import gzip
import re
import shutil
import subprocess

import pytest

import hast_amd
from tests.conftest import load_case, run_s00_case
from tests.test_cli_kc_ingest_gpu import ingest_line, on_device, totals

pytestmark = pytest.mark.gpu
EXE = hast_amd.unshared_kmers_exe()
CASE = "s00_fasta_k11"
FASTA = ["--table-gb", "0.25", "--ingest", "device", "--device-fasta", "--stats"]
RUNS = ("all", "ge2")


def formats_line(stderr: bytes):
    m = re.search(rb"\[stats\] ingest device formats: fastq_blocks=(\d+) fasta_blocks=(\d+)\n", stderr)
    assert m, stderr[-1500:]
    return int(m.group(1)), int(m.group(2))


def fasta_on_device(res, gz=False):
    blocks = on_device(res, gz)                          # fallback=none, blocks_framed > 0, no "starting over"
    fastq_blocks, fasta_blocks = formats_line(res.stderr)
    assert fasta_blocks > 0 and fastq_blocks + fasta_blocks == blocks, res.stderr[-1500:]
    return blocks


def refold(data: bytes, width=7, brk=b"\r\n"):
    """the same records on `width`-column lines"""
    out = bytearray()
    for rec in data.split(b">")[1:]:
        header, _, rest = rec.partition(b"\n")
        seq = b"".join(l.rstrip(b"\r") for l in rest.split(b"\n"))
        out += b">" + header.rstrip(b"\r") + brk
        for at in range(0, len(seq), width):
            out += seq[at:at + width] + brk
    return bytes(out)


def products_equal_goldens(work, run):
    for prod, rec in load_case(CASE)["runs"][run]["products"].items():
        got = b"".join(sorted(open(work / prod, "rb").read().splitlines(keepends=True)))
        assert got == open(work / rec["expected"], "rb").read(), (run, prod)


@pytest.mark.parametrize("run", RUNS)
def test_fasta_parents_are_framed_on_the_device(golden_workdir, tmp_path, run):
    res = run_s00_case(EXE, golden_workdir, tmp_path, CASE, run, extra_args=FASTA)
    fasta_on_device(res)
    assert formats_line(res.stderr)[0] == 0


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("block", (512, 4096))
def test_in_small_blocks(golden_workdir, tmp_path, monkeypatch, run, block):
    monkeypatch.setenv("HAST_KC_INGEST_BLOCK", str(block))
    res = run_s00_case(EXE, golden_workdir, tmp_path, CASE, run, extra_args=FASTA)
    assert fasta_on_device(res) > (10 if block == 512 else 2)


@pytest.mark.parametrize("run", RUNS)
def test_in_blocks_of_64_bytes_on_7_column_lines(golden_workdir, tmp_path, monkeypatch, run):
    """the goldens' records on 7-column CRLF lines: every 11-mer straddles a line break, and most of them a view boundary too"""
    base = tmp_path / "folded"
    shutil.copytree(golden_workdir / CASE, base / CASE)
    for name in ("m.fa", "p.fa", "p_crlf.fa"):
        (base / CASE / name).write_bytes(refold((base / CASE / name).read_bytes()))
    monkeypatch.setenv("HAST_KC_INGEST_BLOCK", "64")
    res = run_s00_case(EXE, base, tmp_path, CASE, run, extra_args=FASTA)
    assert fasta_on_device(res) > 100


@pytest.mark.parametrize("run", RUNS)
def test_a_line_longer_than_a_block_goes_through_the_host_parser(golden_workdir, tmp_path, monkeypatch, run):
    monkeypatch.setenv("HAST_KC_INGEST_BLOCK", "64")
    res = run_s00_case(EXE, golden_workdir, tmp_path, CASE, run, extra_args=FASTA)           # (compares the products with the goldens)
    _, _, fallback = ingest_line(res.stderr)
    assert "full block" in fallback and b"starting over with the host ingest" in res.stderr


@pytest.mark.parametrize("run", RUNS)
def test_flag_from_the_environment(golden_workdir, tmp_path, monkeypatch, run):
    monkeypatch.setenv("HAST_KC_DEVICE_FASTA", "1")
    res = run_s00_case(EXE, golden_workdir, tmp_path, CASE, run, extra_args=["--table-gb", "0.25", "--ingest", "device", "--stats"])
    fasta_on_device(res)


def test_the_flag_is_ignored_by_the_host_ingest(golden_workdir, tmp_path):
    res = run_s00_case(EXE, golden_workdir, tmp_path, CASE, "all", extra_args=["--table-gb", "0.25", "--ingest", "host", "--device-fasta", "--stats"])
    assert b"ingest device" not in res.stderr


def test_gz_files_cut_inside_a_line_are_one_stream(golden_workdir, tmp_path):
    """the paternal files as ONE stream in two .fa.gz files, the first ending inside a sequence line; its format is decided once"""
    work = tmp_path / "gz"
    shutil.copytree(golden_workdir / CASE, work)
    whole = (work / "p_crlf.fa").read_bytes() + (work / "p.fa").read_bytes()       # the script puts each new file in FRONT of the list
    cut = len(whole) // 2
    while whole[cut - 1] in b">\r\n" or whole[cut] in b">\r\n" or b">" in whole[whole.rfind(b"\n", 0, cut) + 1:cut]:
        cut += 1
    for name, part in (("p_first.fa.gz", whole[:cut]), ("p_second.fa.gz", whole[cut:]), ("m.fa.gz", (work / "m.fa").read_bytes())):
        with gzip.GzipFile(work / name, "wb", mtime=0) as f:
            f.write(part)
    argv = ["--maternal", "m.fa.gz", "--paternal", "p_second.fa.gz", "--paternal", "p_first.fa.gz"] + load_case(CASE)["runs"]["all"]["argv"][6:]
    assert argv[6] == "--mer"
    res = subprocess.run([EXE] + argv + FASTA, cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert res.returncode == 0, res.stderr[-1000:]
    fasta_on_device(res, gz=True)
    assert b"in order" not in res.stderr
    products_equal_goldens(work, "all")


def test_fastq_parents_with_the_flag(golden_workdir, tmp_path):
    res = run_s00_case(EXE, golden_workdir, tmp_path, "s00_trio_k21", "default_bounds", extra_args=FASTA)
    blocks = on_device(res, False)
    assert formats_line(res.stderr) == (blocks, 0)


def test_one_parent_fasta_the_other_fastq(golden_workdir, tmp_path):
    runs = []
    for how in (["--ingest", "host"], ["--ingest", "device", "--device-fasta"]):
        work = tmp_path / how[1]
        shutil.copytree(golden_workdir / CASE, work)
        fq = bytearray()
        for rec in (work / "m.fa").read_bytes().split(b">")[1:]:
            header, _, rest = rec.partition(b"\n")
            seq = rest.replace(b"\n", b"").replace(b"\r", b"")
            fq += b"@" + header + b"\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n"
        (work / "m.fq").write_bytes(bytes(fq))
        argv = ["--maternal", "m.fq"] + load_case(CASE)["runs"]["all"]["argv"][2:] + ["--table-gb", "0.25", "--stats"]
        res = subprocess.run([EXE] + argv + how, cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert res.returncode == 0, res.stderr[-1000:]
        runs.append((work, res))
    (host_dir, host), (dev_dir, dev) = runs
    blocks = on_device(dev, False)
    fastq_blocks, fasta_blocks = formats_line(dev.stderr)
    assert fastq_blocks > 0 and fasta_blocks > 0 and fastq_blocks + fasta_blocks == blocks
    assert totals(host.stderr) == totals(dev.stderr)
    products_equal_goldens(dev_dir, "all")               # (the maternal records are the goldens', whatever their format)
    for prod in ("paternal.unique.filter.mer", "maternal.unique.filter.mer"):
        assert (host_dir / prod).read_bytes() == (dev_dir / prod).read_bytes(), prod


@pytest.mark.parametrize("run", RUNS)
def test_totals_equal_the_host_ingests(golden_workdir, tmp_path, run):
    host = run_s00_case(EXE, golden_workdir, tmp_path / "h", CASE, run, extra_args=["--table-gb", "0.25", "--ingest", "host", "--stats"])
    dev = run_s00_case(EXE, golden_workdir, tmp_path / "d", CASE, run, extra_args=FASTA)
    fasta_on_device(dev)
    assert totals(host.stderr) == totals(dev.stderr)
    assert [l for l in host.stdout.splitlines() if not l.startswith(b"CMD")] == [l for l in dev.stdout.splitlines() if not l.startswith(b"CMD")]


def test_an_input_that_is_neither_format_reads_as_with_the_host_ingest(golden_workdir, tmp_path):
    work = tmp_path / "bad"
    shutil.copytree(golden_workdir / CASE, work)
    (work / "p.fa").write_bytes(b"ACGT\n" + (work / "p.fa").read_bytes())
    argv = load_case(CASE)["runs"]["all"]["argv"] + ["--table-gb", "0.05"]
    runs = [subprocess.run([EXE] + argv + how, cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            for how in (["--ingest", "host"], ["--ingest", "device", "--device-fasta"])]
    errors = [[l for l in r.stdout.splitlines() if l.startswith(b"ERROR:")] for r in runs]
    assert runs[0].returncode == runs[1].returncode == 1 and errors[0] == errors[1] and len(errors[0]) == 1, (errors, runs[1].stderr[-500:])
    assert b"neither '>' nor '@'" in errors[0][0]
