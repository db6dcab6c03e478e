"""GPU test of `fake_10x --convert device --inflate device`: the inputs are inflated on the GPU into the paired feed (hast_tx_feed_*), and
stdout and both outputs are still the script's goldens (tests/golden/fake10x/), the steps are the program's steps, and the stats say
where the inputs were inflated.  A side the GPU cannot inflate goes through the host beside the other; a damaged .gz ends the run
with exit 2."""
import gzip
import os
import re
import subprocess
import zlib

import pytest

import hast_amd
from tests import tx_model as tm

pytestmark = pytest.mark.gpu
BLOCK = {"edge": 100, "widths": 4096, "long": 9000}
OUT = ("--plain-out", "--deflate device", "--deflate host")
STATS = re.compile(rb"\[stats\] transform device: steps=(\d+) pairs_on_device=(\d+) pairs_on_host=(\d+) fallback=(\S+)\n"
                   rb"\[stats\] seconds: upload=[\d.]+ kernels=[\d.]+ deflate=[\d.]+ download=[\d.]+ write=[\d.]+ read_phase=[\d.]+ plain_in_bytes=(\d+) out_bytes=\d+\+\d+\n"
                   rb"\[stats\] ingest device: gz_on_device=(\d) host_sides=(\d) steps_on_host=(\d+) collect_wait=[\d.]+ fallback=(\S+)\n")


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


class Ran:
    pass


def run_feed(d, files, map_text, block, out_mode, env=None, extra=("--convert", "device", "--inflate", "device"), want_rc=0):
    """fake_10x in directory d over files = ((name, bytes on disk), (name, bytes on disk))"""
    d.mkdir()
    args = [files[0][0], files[1][0], "map.txt"]
    for name, data in files:
        (d / name).write_bytes(data)
    (d / "map.txt").write_bytes(map_text)
    r = subprocess.run([hast_amd.fake_10x_exe()] + args + ["--stats"] + list(extra) + out_mode.split(), cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, HAST_TX_BLOCK=str(block), **(env or {})), timeout=300)
    assert r.returncode == want_rc, (r.returncode, r.stderr)
    ran = Ran()
    ran.args, ran.stdout, ran.stderr = args, r.stdout, r.stderr
    if want_rc:
        return ran
    ran.raw = [(d / ("SampleName_S1_L001_R%d_001.fastq%s" % (side, "" if out_mode == "--plain-out" else ".gz"))).read_bytes() for side in (1, 2)]
    ran.outs = ran.raw if out_mode == "--plain-out" else [gzip.decompress(x) if x else b"" for x in ran.raw]
    m = STATS.search(r.stderr)
    assert m, r.stderr
    ran.steps, ran.on_device, ran.on_host, ran.plain_in, ran.gz_on_device, ran.host_sides, ran.steps_on_host = (int(m.group(i)) for i in (1, 2, 3, 5, 6, 7, 8))
    ran.fallback, ran.feed_fallback = m.group(4).decode(), m.group(9).decode()
    return ran


def check_golden(ran, case, out_mode):
    r1, r2, map_text = (tm.golden(case, n) for n in ("r1.fq", "r2.fq", "map.txt"))
    assert ran.stdout == tm.banner(*ran.args) + tm.golden(case, "stdout.txt")[len(tm.banner(*tm.GOLDEN_ARGS)):]
    assert ran.outs[0] == tm.golden(case, "out1.fq") and ran.outs[1] == tm.golden(case, "out2.fq")
    assert ran.on_device + ran.on_host == int(re.search(rb"Total (\d+) pair", ran.stdout).group(1))
    assert ran.fallback == "none" and ran.feed_fallback == "none" and b"WARN" not in ran.stderr
    assert ran.plain_in == len(r1) + len(r2)
    want_steps, want_runs = steps_of_the_program(r1, r2, map_text, BLOCK[case])
    assert ran.steps == want_steps
    if case == "edge":
        assert ran.on_device >= 1
    else:
        assert ran.on_host <= 1 and ran.steps > 4                   # the closing step at most is the host's
    if out_mode == "--deflate device":
        for side in range(2):
            parts = members(ran.raw[side])
            assert len(parts) == want_runs[side] and all(parts) and b"".join(parts) == ran.outs[side]


def gz_files(case):
    return (("r1.fq.gz", gzip.compress(tm.golden(case, "r1.fq"))), ("r2.fq.gz", gzip.compress(tm.golden(case, "r2.fq"))))


@pytest.mark.parametrize("out_mode", OUT)
@pytest.mark.parametrize("case", ("edge", "widths", "long"))
def test_feed_route_reproduces_the_script(tmp_path, case, out_mode):
    ran = run_feed(tmp_path / "w", gz_files(case), tm.golden(case, "map.txt"), BLOCK[case], out_mode)
    check_golden(ran, case, out_mode)
    assert (ran.gz_on_device, ran.host_sides) == (2, 0)


@pytest.mark.parametrize("case", ("edge", "widths", "long"))
def test_feed_route_over_several_decode_passes(tmp_path, case):
    """chunks of 1 KB, three a pass: the inputs' inflate takes several passes of the decoder, blocks span them"""
    ran = run_feed(tmp_path / "w", gz_files(case), tm.golden(case, "map.txt"), BLOCK[case], "--deflate device",
                   env={"HAST_GZ_CHUNK_BYTES": "1024", "HAST_GZ_PASS_CHUNKS": "3"})
    check_golden(ran, case, "--deflate device")
    assert (ran.gz_on_device, ran.host_sides) == (2, 0)


@pytest.mark.parametrize("plain_side", (0, 1))
def test_one_side_gz_and_the_other_plain(tmp_path, plain_side):
    case = "widths"
    files = [("r%d.fq" % (s + 1), tm.golden(case, "r%d.fq" % (s + 1))) if s == plain_side else gz_files(case)[s] for s in range(2)]
    ran = run_feed(tmp_path / "w", files, tm.golden(case, "map.txt"), BLOCK[case], "--deflate device")
    check_golden(ran, case, "--deflate device")
    assert (ran.gz_on_device, ran.host_sides) == (1, 1)


def test_read_1_as_two_members_cut_inside_a_record(tmp_path):
    case = "long"
    r1 = tm.golden(case, "r1.fq")
    cut = r1.index(b"\n", len(r1) // 2) + 3                          # behind a newline and two more bytes: inside a line
    files = (("r1.fq.gz", gzip.compress(r1[:cut]) + gzip.compress(r1[cut:])), gz_files(case)[1])
    ran = run_feed(tmp_path / "w", files, tm.golden(case, "map.txt"), BLOCK[case], "--deflate device")
    check_golden(ran, case, "--deflate device")
    assert (ran.gz_on_device, ran.host_sides) == (2, 0)


@pytest.mark.parametrize("n1,n2", ((300, 10), (10, 300), (0, 5), (5, 0)))
def test_feed_route_on_inputs_of_different_lengths(tmp_path, n1, n2):
    """read 2 ends first: the script goes on through read 1 and pairs it with nothing; read 1 ends first: the rest of read 2 is ignored"""
    r1 = b"".join(b"@a%d#k/1\n%s\n+\n%s\n" % (i, b"ACGT" * 6, b"!III" * 6) for i in range(n1))
    r2 = b"".join(b"@a%d#k/2\n%s\n+\n%s\n" % (i, b"TTGCA" * 5, b"FFFF!" * 5) for i in range(n2)) + (b"@cut#k/2\nTT" if n2 == 10 else b"")
    want1, want2, log, used, _ = tm.convert({b"k": b"ACGTACGTACGTACGT"}, r1, r2)
    assert used == n1
    map_text = b"k\tACGTACGTACGTACGT\n"
    ran = run_feed(tmp_path / "w", (("r1.fq.gz", gzip.compress(r1)), ("r2.fq.gz", gzip.compress(r2))), map_text, 256, "--deflate device")
    assert ran.stdout == tm.banner(*ran.args) + log and (ran.outs[0], ran.outs[1]) == (want1, want2)
    assert ran.on_device + ran.on_host == n1 and ran.fallback == "none" and ran.feed_fallback == "none"
    assert ran.steps == steps_of_the_program(r1, r2, map_text, 256)[0]
    if min(n1, n2) >= 10:
        assert ran.on_device >= 8                                    # the pairs both inputs hold whole go to the device


@pytest.mark.parametrize("damage", ("truncated", "bit"))
def test_a_damaged_gz_is_exit_2(tmp_path, damage):
    case = "long"
    z = bytearray(gzip.compress(tm.golden(case, "r2.fq")))
    if damage == "truncated":
        z = z[:len(z) // 2]
    else:
        z[len(z) // 2] ^= 0x10
    ran = run_feed(tmp_path / "w", (gz_files(case)[0], ("r2.fq.gz", bytes(z))), tm.golden(case, "map.txt"), BLOCK[case], "--deflate device", want_rc=2)
    assert b"r2.fq.gz" in ran.stderr


def test_inflate_device_needs_convert_device(tmp_path):
    ran = run_feed(tmp_path / "w", gz_files("edge"), tm.golden("edge", "map.txt"), 100, "--plain-out", extra=("--inflate", "device"), want_rc=1)
    assert b"usage" in ran.stderr


def test_a_map_the_device_cannot_take_goes_the_host_way(tmp_path):
    case = "fb_key16"
    ran = run_feed(tmp_path / "w", gz_files(case), tm.golden(case, "map.txt"), 100, "--deflate host")
    assert ran.outs[0] == tm.golden(case, "out1.fq") and ran.outs[1] == tm.golden(case, "out2.fq")
    reason = tm.FALLBACK[case][1].replace(" ", "_")
    assert b"WARN" in ran.stderr and ran.on_device == 0 and ran.fallback == reason and ran.feed_fallback == reason
    assert (ran.gz_on_device, ran.host_sides, ran.steps_on_host) == (0, 2, 0)
