"""GPU test of `fake_10x --convert device`: on the goldens the script wrote (tests/golden/fake10x/) its stdout and both outputs are the
script's, whatever the input and output formats; the steps over whole pairs really run on the device (the stats line counts the
pairs per route, and well-formed inputs leave the host the closing step at most); a map the device cannot take sends the run the host
way and says why."""
import gzip
import os
import re
import subprocess
import zlib

import pytest

import hast_amd
from tests import tx_model as tm

pytestmark = pytest.mark.gpu
CASES = ("edge", "widths", "long", "fb_value17", "fb_key16", "fb_emptykey")
BLOCK = {"edge": 100, "widths": 4096, "long": 9000}
OUT = ("--plain-out", "--deflate device", "--deflate host")
STATS = re.compile(rb"\[stats\] transform device: steps=(\d+) pairs_on_device=(\d+) pairs_on_host=(\d+) fallback=(\S+)\n"
                   rb"\[stats\] seconds: upload=[\d.]+ kernels=[\d.]+ deflate=[\d.]+ download=[\d.]+ write=[\d.]+ ")


@pytest.fixture(scope="module")
def lib():
    return hast_amd.lib()


def members(data):
    """the gzip members of a file, each inflated"""
    out = []
    while data:
        d = zlib.decompressobj(31)
        out.append(d.decompress(data))
        assert d.eof
        data = d.unused_data
    return out


def steps_of_the_program(r1, r2, map_text, block):
    """the program's steps over these inputs, from its reading rule and the host model -> (steps, steps with a non-empty run per side)"""
    lib = hast_amd.lib()
    src, have, at, eof = (r1, r2), [b"", b""], [0, 0], [False, False]
    steps, runs, mode, st = 0, [0, 0], 0, hast_amd.TxState(0, 0)
    with hast_amd.TxMap(map_text) as m:
        while mode != 1:
            for s in range(2):
                # a side that has more than a block waiting, a whole record in it, reads nothing
                if eof[s] or (len(have[s]) > block and have[s].count(b"\n") >= 4):
                    continue
                piece = src[s][at[s]:at[s] + block]
                at[s] += len(piece)
                have[s] += piece
                eof[s] = len(piece) < block
            mode = lib.hast_tx_step_mode(eof[0], eof[1], have[0], len(have[0]), have[1], len(have[1]))
            o1, o2, res = m.pair_host(have[0], have[1], mode, st)
            steps += 1
            runs = [runs[0] + bool(o1), runs[1] + bool(o2)]
            have = [have[0][res.consumed1:], have[1][res.consumed2:]]
    return steps, runs


def run_device(d, r1, r2, map_text, gz_in, block, out_mode):
    """fake_10x --convert device in directory d -> (stdout, out1, out2, (steps, D, H, fallback), args, the raw output files)"""
    d.mkdir()
    args = ["r1.fq.gz", "r2.fq.gz", "map.txt"] if gz_in else ["r1.fq", "r2.fq", "map.txt"]
    for name, data in zip(args, (r1, r2)):
        with (gzip.open(d / name, "wb") if gz_in else open(d / name, "wb")) as f:
            f.write(data)
    (d / "map.txt").write_bytes(map_text)
    r = subprocess.run([hast_amd.fake_10x_exe()] + args + ["--stats", "--convert", "device"] + out_mode.split(), cwd=d, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, env=dict(os.environ, HAST_TX_BLOCK=str(block)), timeout=300)
    assert r.returncode == 0, r.stderr
    raw = [(d / ("SampleName_S1_L001_R%d_001.fastq%s" % (side, "" if out_mode == "--plain-out" else ".gz"))).read_bytes() for side in (1, 2)]
    outs = raw if out_mode == "--plain-out" else [gzip.decompress(x) if x else b"" for x in raw]
    m = STATS.search(r.stderr)
    assert m, r.stderr
    return r.stdout, outs[0], outs[1], (int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4).decode()), args, raw, r.stderr


@pytest.mark.parametrize("out_mode", OUT)
@pytest.mark.parametrize("gz_in", (True, False), ids=("gz", "plain"))
@pytest.mark.parametrize("case", CASES)
def test_device_route_reproduces_the_script(lib, tmp_path, case, gz_in, out_mode):
    out, o1, o2, (steps, on_device, on_host, fallback), args, raw, err = run_device(
        tmp_path / "w", tm.golden(case, "r1.fq"), tm.golden(case, "r2.fq"), tm.golden(case, "map.txt"), gz_in, BLOCK.get(case, 100), out_mode)
    assert out == tm.banner(*args) + tm.golden(case, "stdout.txt")[len(tm.banner(*tm.GOLDEN_ARGS)):]
    assert o1 == tm.golden(case, "out1.fq") and o2 == tm.golden(case, "out2.fq")
    assert on_device + on_host == int(re.search(rb"Total (\d+) pair", out).group(1))
    if case in tm.FALLBACK:
        assert on_device == 0 and fallback == tm.FALLBACK[case][1].replace(" ", "_") and b"WARN" in err
        return
    assert fallback == "none" and b"WARN" not in err
    if case == "edge":
        assert on_device >= 1
    else:
        assert on_host <= 1 and steps > 4                       # the closing step at most is the host's: this cannot pass on the host route
    if out_mode == "--deflate device":
        # one member per step and side that had something to write (an empty run is no member), each one what Python's gzip reads
        want_steps, want_runs = steps_of_the_program(tm.golden(case, "r1.fq"), tm.golden(case, "r2.fq"), tm.golden(case, "map.txt"), BLOCK.get(case, 100))
        assert steps == want_steps
        for side in range(2):
            parts = members(raw[side])
            assert len(parts) == want_runs[side] and all(parts) and b"".join(parts) == (o1, o2)[side]
            if case != "edge":
                assert len(parts) > 4


@pytest.mark.parametrize("n1,n2", ((300, 10), (10, 300), (0, 5), (5, 0)))
def test_device_route_on_inputs_of_different_lengths(lib, tmp_path, n1, n2):
    """read 2 ends first: the script goes on through read 1 and pairs it with nothing; read 1 ends first: the rest of read 2 is ignored"""
    r1 = b"".join(b"@a%d#k/1\n%s\n+\n%s\n" % (i, b"ACGT" * 6, b"!III" * 6) for i in range(n1))
    r2 = b"".join(b"@a%d#k/2\n%s\n+\n%s\n" % (i, b"TTGCA" * 5, b"FFFF!" * 5) for i in range(n2)) + (b"@cut#k/2\nTT" if n2 == 10 else b"")
    want1, want2, log, used, _ = tm.convert({b"k": b"ACGTACGTACGTACGT"}, r1, r2)
    assert used == n1
    out, o1, o2, (steps, on_device, on_host, fallback), args, raw, err = run_device(tmp_path / "w", r1, r2, b"k\tACGTACGTACGTACGT\n", True, 256, "--deflate device")
    assert out == tm.banner(*args) + log and (o1, o2) == (want1, want2)
    assert on_device + on_host == n1 and fallback == "none"
    if min(n1, n2) >= 10:
        assert on_device >= 8                                    # the pairs both inputs hold whole go to the device
