"""quartering_fastq --gz-out --gz-format bgzf (the host twin of the device encoder's blocked mode; hast_amd/csrc/quartering.h
bgzf_members) against the outputs of the reference's awk program: the four files inflate (Python's gzip module) to the plain files
byte for byte, EVERY member of them is BGZF (18-byte header with the BC subfield, at most 64 KB, at most 49 152 bytes inflated),
each file ends with exactly one end-of-file block and holds no other empty member, a class nothing is routed to gets no file.
Without the flag the files are what --gz-out alone writes, byte for byte; a bad value, or the flag without --gz-out, is exit 255."""
import gzip
import hashlib
import json
import os
import shutil
import subprocess

import pytest

import hast_amd
from tests.conftest import GOLDEN
from tests.test_dz_blocked_cpu import EOF_BLOCK, MEMBER_INPUT, walk_members
from tests.test_quartering_cpu import EXE

LISTS = ["paternal.unique.barcodes", "maternal.unique.barcodes", "homozygous.unique.barcodes"]
CLASSES = ("paternal", "maternal", "homozygous", "nobarcode")


@pytest.fixture(scope="module")
def exe():
    hast_amd.build()
    return EXE


def check_bgzf_file(blob, plain):
    """blob: whole BGZF members that inflate to plain, none of more than 49 152 bytes; the last one is the end-of-file block and no
    other member is empty.  Returns the number of members."""
    members = walk_members(blob)
    assert gzip.decompress(blob) == plain
    assert blob[-28:] == EOF_BLOCK
    sizes = [isize for _, _, _, isize in members]
    assert sizes[-1] == 0 and all(0 < s <= MEMBER_INPUT for s in sizes[:-1]) and sum(sizes) == len(plain)
    return len(members)


def rand_k21_inputs(tmp_path, exp):
    for name in ("paternal", "maternal", "homozygous"):
        shutil.copy(os.path.join(GOLDEN, "quartering", name + ".unique.barcodes"), tmp_path)
    out = {}
    for fq in ("r1.fq", "r2.fq"):
        data = gzip.open(os.path.join(GOLDEN, "rand_k21", fq + ".gz")).read()
        if fq == "r2.fq":
            data = data[:-1] + b"\n" + exp["r2_tail"].encode()
        (tmp_path / fq).write_bytes(data)
        out[fq] = data
    return out


def test_edge_case_all_branches_as_bgzf(exe, tmp_path):
    exp = json.load(open(os.path.join(GOLDEN, "quartering", "expected.json")))["edge"]
    for fn, txt in exp["inputs"].items():
        (tmp_path / fn).write_text(txt)
    on_disk = {fn: fn + ".gz" if fn.endswith(".fastq") else fn for fn in exp["outputs"]}
    for threads in (1, 5):
        for fn in on_disk.values():
            (tmp_path / fn).unlink(missing_ok=True)
        r = subprocess.run([exe, "-t", str(threads), "--gz-out", "--gz-format", "bgzf", "--prefix", "e.fq", "p.bc", "m.bc", "h.bc", "e.fq"], cwd=tmp_path,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0 and r.stdout == b""
        assert r.stderr.decode() == exp["stderr"]
        for fn, d in on_disk.items():
            if d == fn:
                assert (tmp_path / d).read_text() == exp["outputs"][fn]
            else:
                check_bgzf_file((tmp_path / d).read_bytes(), exp["outputs"][fn].encode())
        assert sorted(os.listdir(tmp_path)) == sorted(list(exp["inputs"]) + list(on_disk.values()))


@pytest.mark.parametrize("threads,block_mb", [(1, 64), (8, 1)])
def test_rand_k21_as_bgzf_matches_reference_awk(exe, tmp_path, threads, block_mb):
    exp = json.load(open(os.path.join(GOLDEN, "quartering", "expected.json")))
    rand_k21_inputs(tmp_path, exp)
    n_members = 0
    for fq in ("r1.fq", "r2.fq"):
        r = subprocess.run([exe, "-t", str(threads), "--block-mb", str(block_mb), "--gz-out", "--gz-format", "bgzf", "--prefix", fq] + LISTS + [fq], cwd=tmp_path,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()[-500:]
        e = exp["files"][fq]
        assert hashlib.md5(r.stderr).hexdigest() == e["stderr_md5"]
        for cls in CLASSES:
            p = tmp_path / ("%s.%s.fastq.gz" % (fq, cls))
            assert not (tmp_path / ("%s.%s.fastq" % (fq, cls))).exists()
            if cls in e:
                z = p.read_bytes()
                b = gzip.decompress(z)
                assert (len(b), hashlib.md5(b).hexdigest()) == (e[cls]["bytes"], e[cls]["md5"]), (fq, cls)
                n_members += check_bgzf_file(z, b)
                assert len(z) < len(b)
            else:
                assert not p.exists()
    assert n_members > 8                                    # (runs of more than 49 152 bytes: several members a worker's share)
    assert (tmp_path / "filter_reads.log").read_text() == exp["filter_reads_log"]


def test_without_the_flag_and_with_gzip_the_files_are_those_of_gz_out_alone(exe, tmp_path):
    exp = json.load(open(os.path.join(GOLDEN, "quartering", "expected.json")))
    got = {}
    for how in ("alone", "gzip"):
        d = tmp_path / how
        d.mkdir()
        rand_k21_inputs(d, exp)
        for fq in ("r1.fq", "r2.fq"):
            r = subprocess.run([exe, "-t", "3", "--block-mb", "1", "--gz-out"] + (["--gz-format", "gzip"] if how == "gzip" else []) + ["--prefix", fq] + LISTS + [fq], cwd=d,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            assert r.returncode == 0, r.stderr.decode()[-500:]
        got[how] = {fn: (d / fn).read_bytes() for fn in sorted(os.listdir(d)) if fn.endswith(".fastq.gz")}
    assert len(got["alone"]) >= 6 and got["alone"] == got["gzip"]
    for fn, z in got["alone"].items():
        assert z[:4] == b"\x1f\x8b\x08\x00" and z[-28:] != EOF_BLOCK, fn      # ordinary members, no end-of-file block


@pytest.mark.parametrize("flags", [["--gz-out", "--gz-format", "foo"], ["--gz-out", "--gz-format", ""], ["--gz-format", "bgzf"], ["--gz-format", "gzip"]])
def test_a_bad_value_exits_255(exe, tmp_path, flags):
    exp = json.load(open(os.path.join(GOLDEN, "quartering", "expected.json")))["edge"]
    for fn, txt in exp["inputs"].items():
        (tmp_path / fn).write_text(txt)
    before = sorted(os.listdir(tmp_path))
    r = subprocess.run([exe] + flags + ["--prefix", "e.fq", "p.bc", "m.bc", "h.bc", "e.fq"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 255 and b"usage" in r.stderr and b"--gz-format" in r.stderr
    assert sorted(os.listdir(tmp_path)) == before           # (nothing was read or written)
