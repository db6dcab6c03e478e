"""Host-only tests of the stLFR -> 10x conversion (stage 02, fake_10x.pl): the rules of hast_amd/csrc/tx_core.h as the C host model
(tx_host.h, stepped by tests/native/test_tx_core.cpp the way the fake_10x program feeds it, and behind hast_tx_pair_host) and as a
short Python restatement (tests/tx_model.py), both held to what the script itself wrote (tests/golden/fake10x/)."""
import os
import re
import subprocess

import pytest

import hast_amd
from tests import tx_model as tm
from tests.conftest import ROOT

CASES = ("edge", "widths", "long", "fb_value17", "fb_key16", "fb_emptykey")
BLOCKS = (64, 100, 700, 4096, 65536)
REASONS = dict({c: "none" for c in CASES}, **{c: reason for c, (_, reason) in tm.FALLBACK.items()})


golden = tm.golden


def build_native(out_dir, sanitize):
    """tests/native/test_tx_core.cpp as a stand-alone program, optionally under ASan + UBSan"""
    out = os.path.join(str(out_dir), "test_tx_core_san" if sanitize else "test_tx_core")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra"] + (["-fsanitize=address,undefined"] if sanitize else []) + \
          ["-o", out, os.path.join(ROOT, "tests", "native", "test_tx_core.cpp")]
    subprocess.run(cmd, check=True)
    return out


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("tx_core")


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def driver(request, work):
    return build_native(work, request.param == "asan_ubsan")


@pytest.fixture(scope="module")
def lib():
    hast_amd.build()
    return hast_amd.lib()


@pytest.mark.parametrize("case", CASES)
def test_python_model_reproduces_the_script(case):
    m = tm.parse_map(golden(case, "map.txt"))
    out1, out2, log, _, _ = tm.convert(m, golden(case, "r1.fq"), golden(case, "r2.fq"))
    assert out1 == golden(case, "out1.fq") and out2 == golden(case, "out2.fq")
    assert tm.banner(*tm.GOLDEN_ARGS) + log == golden(case, "stdout.txt")
    assert tm.device_ok(m) == (REASONS[case] == "none", REASONS[case])


def test_the_script_said_what_the_issue_quotes():
    assert golden("edge", "stdout.txt").endswith(b"Total 13 pair reads and used 7 pairs.\n")
    assert b"\nTotal 1200 pair reads and used 1190 pairs.\n" in golden("widths", "stdout.txt")          # N crosses 9, 99 and 999


def test_key_rule_table():
    rows = {b"@r#A_1/1\tx": b"A_1", b"@r#A_1#zz/1": b"A_1", b"@r/1#A_1": b"A_1", b"@r\t#A_1/1": b"", b"@r#A_1\r": b"A_1\r", b"@r#A_1 /1": b"A_1 ",
            b"@r#/1": b"", b"@r#": b"", b"@r": b""}
    for head, key in rows.items():
        assert tm.key_of(head) == key, head
    # the C rule, through the model: a map that holds exactly the expected key keeps the pair, any other drops it
    hast_amd.build()
    for head, key in rows.items():
        for probe, kept in ((key, True), (key + b"x", False)):
            with hast_amd.TxMap(probe + b"\tV\n") as m:
                st = hast_amd.TxState(0, 0)
                o1, _, res = m.pair_host(head + b"\nAC\n+\nII\n", b"@q\nGT\n+\n!I\n", True, st)
                assert (res.used == 1) == kept and st.headers == 1, (head, probe)
                if kept:
                    assert o1 == b"@ST-E0:0:SIMULATE:8:0:0:1 1:N:0:NAAGTGCT\nVATCGAGNAC\n+\n" + b"F" * 22 + b"#II\n"


@pytest.mark.parametrize("block", BLOCKS)
def test_native_model_reproduces_the_script_at_every_block_size(driver, work, block):
    for case in CASES:
        o1, o2 = str(work / "o1.fq"), str(work / "o2.fq")
        args = [str(work / name) for name in ("r1.fq", "r2.fq", "map.txt")]
        for path, name in zip(args, ("r1.fq", "r2.fq", "map.txt")):
            open(path, "wb").write(golden(case, name))
        r = subprocess.run([driver, "-b", str(block)] + args + [o1, o2], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0 and b"runtime error" not in r.stderr and b"Sanitizer" not in r.stderr, r.stderr.decode()[-2000:]
        assert open(o1, "rb").read() == golden(case, "out1.fq") and open(o2, "rb").read() == golden(case, "out2.fq"), (case, block)
        want = golden(case, "stdout.txt")[len(tm.banner(*tm.GOLDEN_ARGS)):]
        assert r.stdout == tm.banner(*args) + want, (case, block)
        ok = REASONS[case] == "none"
        assert ("device_ok=%d reason=%s\n" % (ok, REASONS[case])).encode() in r.stderr, r.stderr
        if block <= 700 and case in ("widths", "long"):
            assert int(r.stderr.split(b"steps=")[1]) > 4


@pytest.mark.parametrize("case", CASES)
def test_map_parsing_through_the_abi(lib, case):
    text = golden(case, "map.txt")
    with hast_amd.TxMap(text) as m:
        assert m.n_keys == len(tm.parse_map(text))
        assert (m.device_ok, m.reason) == (REASONS[case] == "none", REASONS[case])
        st = hast_amd.TxState(0, 0)
        o1, o2, res = m.pair_host(golden(case, "r1.fq"), golden(case, "r2.fq"), True, st)
        assert o1 == golden(case, "out1.fq") and o2 == golden(case, "out2.fq")
        assert b"Total %d pair reads and used %d pairs.\n" % (st.headers, st.used) in golden(case, "stdout.txt")


def test_host_model_carries_its_running_state(lib):
    """N and the header count go in and come out: a second call goes on where the first stopped, also across 2^32"""
    with hast_amd.TxMap(b"k\tACGT\n") as m:
        pair = (b"@a#k/1\nAC\n+\n!I\n", b"@a#k/2\nGT\n+\nI!\n")
        for start in (8, 98, 999998, 4294967290, 9999999995):
            st = hast_amd.TxState(start, start + 5)
            o1, o2, res = m.pair_host(pair[0] * 12 + b"@tail", pair[1] * 12, False, st)
            assert (res.pairs, res.used, res.consumed1, res.consumed2) == (12, 12, 12 * len(pair[0]), 12 * len(pair[1]))
            assert (st.used, st.headers) == (start + 12, start + 17)
            want1, want2, _, _, _ = tm.convert({b"k": b"ACGT"}, pair[0] * 12, pair[1] * 12, used=start)
            assert (o1, o2) == (want1, want2)


def run_program(d, r1, r2, map_text, gz_in, block, extra=()):
    """fake_10x in directory d on the given inputs -> (stdout, out1, out2, stderr); the outputs decompressed"""
    import gzip
    d.mkdir()
    args = ["r1.fq.gz", "r2.fq.gz", "map.txt"] if gz_in else ["r1.fq", "r2.fq", "map.txt"]
    for name, data in zip(args, (r1, r2)):
        with (gzip.open(d / name, "wb") if gz_in else open(d / name, "wb")) as f:
            f.write(data)
    (d / "map.txt").write_bytes(map_text)
    r = subprocess.run([hast_amd.fake_10x_exe()] + args + ["--stats"] + list(extra), cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, HAST_TX_BLOCK=str(block)), timeout=300)
    assert r.returncode == 0, r.stderr
    outs = []
    for side in (1, 2):
        p = d / ("SampleName_S1_L001_R%d_001.fastq" % side)
        outs.append(open(p, "rb").read() if "--plain-out" in extra else gzip.open(str(p) + ".gz").read())
    return r.stdout, outs[0], outs[1], r.stderr, args


@pytest.mark.parametrize("gz_in", (True, False), ids=("gz", "plain"))
@pytest.mark.parametrize("case", CASES)
def test_program_reproduces_the_script(lib, tmp_path, case, gz_in):
    """stdout and both outputs, byte for byte, over many steps: blocks far smaller than the inputs, and than `long`'s records"""
    extra = () if gz_in else ("--plain-out", "--inflate", "zlib")
    out, o1, o2, err, args = run_program(tmp_path / "w", golden(case, "r1.fq"), golden(case, "r2.fq"), golden(case, "map.txt"), gz_in,
                                         {"edge": 100, "long": 9000}.get(case, 4096 if case == "widths" else 100), extra)
    assert out == tm.banner(*args) + golden(case, "stdout.txt")[len(tm.banner(*tm.GOLDEN_ARGS)):]
    assert o1 == golden(case, "out1.fq") and o2 == golden(case, "out2.fq")
    headers = int(re.search(rb"Total (\d+) pair", out).group(1))
    m = re.search(rb"\[stats\] transform host: steps=(\d+) pairs_on_device=0 pairs_on_host=(\d+) fallback=none\n", err)
    assert m and int(m.group(1)) > 4 and int(m.group(2)) == headers, err


@pytest.mark.parametrize("n1,n2", ((300, 10), (10, 300), (0, 5), (5, 0)))
def test_program_on_inputs_of_different_lengths(lib, tmp_path, n1, n2):
    """read 2 ends first: the script goes on through read 1 and pairs it with nothing; read 1 ends first: the rest of read 2 is ignored"""
    r1 = b"".join(b"@a%d#k/1\n%s\n+\n%s\n" % (i, b"ACGT" * 6, b"!III" * 6) for i in range(n1))
    r2 = b"".join(b"@a%d#k/2\n%s\n+\n%s\n" % (i, b"TTGCA" * 5, b"FFFF!" * 5) for i in range(n2)) + (b"@cut#k/2\nTT" if n2 == 10 else b"")
    want1, want2, log, used, _ = tm.convert({b"k": b"ACGTACGTACGTACGT"}, r1, r2)
    assert used == n1
    out, o1, o2, err, args = run_program(tmp_path / "w", r1, r2, b"k\tACGTACGTACGTACGT\n", True, 256)
    assert out == tm.banner(*args) + log and (o1, o2) == (want1, want2)


def test_program_refuses_what_it_cannot_read(lib, tmp_path):
    (tmp_path / "map.txt").write_bytes(b"k\tACGT\n")
    (tmp_path / "r1.fq").write_bytes(b"@a#k/1\nAC\n+\nII\n")
    (tmp_path / "bad.fq.gz").write_bytes(b"\x1f\x8b\x08\x00" + b"\x00" * 40)
    for r2, word in (("nothing_here.fq.gz", b"cannot open"), ("bad.fq.gz", b"bad.fq.gz")):
        r = subprocess.run([hast_amd.fake_10x_exe(), "r1.fq", r2, "map.txt"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 2 and word in r.stderr, (r.returncode, r.stderr)
