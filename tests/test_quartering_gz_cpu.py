"""quartering_fastq --gz-out (the host tool; hast_amd/csrc/quartering.h) against the outputs of the reference's awk program: the four
files come out as <prefix>.<class>.fastq.gz -- concatenated gzip members -- whose inflated bytes are the plain files' byte for byte;
stderr and filter_reads.log are what they are without the flag; a class nothing is routed to gets no file; no plain file is left."""
import gzip
import hashlib
import json
import os
import shutil
import subprocess

import pytest

import hast_amd
from tests.conftest import GOLDEN
from tests.test_quartering_cpu import EXE


@pytest.fixture(scope="module")
def exe():
    hast_amd.build()
    return EXE


def test_edge_case_all_branches_as_gzip(exe, tmp_path):
    exp = json.load(open(os.path.join(GOLDEN, "quartering", "expected.json")))["edge"]
    for fn, txt in exp["inputs"].items():
        (tmp_path / fn).write_text(txt)
    on_disk = {fn: fn + ".gz" if fn.endswith(".fastq") else fn for fn in exp["outputs"]}       # (filter_reads.log stays as it is)
    for threads in (1, 5):
        for fn in on_disk.values():
            (tmp_path / fn).unlink(missing_ok=True)
        r = subprocess.run([exe, "-t", str(threads), "--gz-out", "--prefix", "e.fq", "p.bc", "m.bc", "h.bc", "e.fq"], cwd=tmp_path,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0 and r.stdout == b""
        assert r.stderr.decode() == exp["stderr"]
        got = {fn: (gzip.decompress((tmp_path / d).read_bytes()).decode() if d != fn else (tmp_path / d).read_text()) for fn, d in on_disk.items()}
        assert got == exp["outputs"]
        assert sorted(os.listdir(tmp_path)) == sorted(list(exp["inputs"]) + list(on_disk.values()))


@pytest.mark.parametrize("threads,block_mb,via", [(1, 64, "file"), (8, 1, "file"), (3, 1, "gz")])
def test_rand_k21_as_gzip_matches_reference_awk(exe, tmp_path, threads, block_mb, via):
    exp = json.load(open(os.path.join(GOLDEN, "quartering", "expected.json")))
    for name in ("paternal", "maternal", "homozygous"):
        shutil.copy(os.path.join(GOLDEN, "quartering", name + ".unique.barcodes"), tmp_path)
    lists = ["paternal.unique.barcodes", "maternal.unique.barcodes", "homozygous.unique.barcodes"]
    for fq in ("r1.fq", "r2.fq"):
        data = gzip.open(os.path.join(GOLDEN, "rand_k21", fq + ".gz")).read()
        if fq == "r2.fq":
            data = data[:-1] + b"\n" + exp["r2_tail"].encode()
        cmd = [exe, "-t", str(threads), "--block-mb", str(block_mb), "--gz-out", "--prefix", fq] + lists
        if via == "gz":
            with gzip.open(tmp_path / (fq + ".gz"), "wb") as f:
                f.write(data)
            r = subprocess.run(cmd + [fq + ".gz"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        else:
            (tmp_path / fq).write_bytes(data)
            r = subprocess.run(cmd + [fq], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()[-500:]
        e = exp["files"][fq]
        assert hashlib.md5(r.stderr).hexdigest() == e["stderr_md5"]
        for cls in ("paternal", "maternal", "homozygous", "nobarcode"):
            p = tmp_path / ("%s.%s.fastq.gz" % (fq, cls))
            assert not (tmp_path / ("%s.%s.fastq" % (fq, cls))).exists()
            if cls in e:
                z = p.read_bytes()
                b = gzip.decompress(z)
                assert (len(b), hashlib.md5(b).hexdigest()) == (e[cls]["bytes"], e[cls]["md5"]), (fq, cls)
                assert len(z) < len(b)
            else:
                assert not p.exists()
    log = (tmp_path / "filter_reads.log").read_text()
    if via == "file":
        assert log == exp["filter_reads_log"]
    else:
        strip = lambda t: [l for l in t.splitlines() if l.startswith("#")]
        assert strip(log) == strip(exp["filter_reads_log"])
