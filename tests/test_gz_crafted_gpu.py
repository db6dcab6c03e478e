"""The device inflate (hast_gz_*, hast_amd/csrc/gz_kernels.hip) on deflate streams zlib's encoder never writes
(tests/gz_crafted_corpus.py), against zlib's bytes.  What the suite's other streams -- all written by zlib's deflate -- never reach
in the kernels: markers kMarker + i with i < 262, i.e. the oldest bytes of a window (the shifted region of k_gz_maps, the hand-over
from group to group in k_gz_carry, k_gz_window, prev[x - kMarker] in k_gz_crc and k_gz_translate); distance 32 768 in k_gz_decode's
token words; a step that starts at a token with both codes in the second-level tables; a 48-bit token at a high lane offset; a block
without distance codes; a chunk that starts with a long match at distance 32 768 (nothing but markers).  And the forged members:
matches that reach in front of their member's first byte, with the trailer of the bytes that reach would give -- on the device the
window in front of a member is zeros (k_gz_maps), hence the forgeries over a history of zeros -- are errors, never other data.
tests/test_inflate_crafted_cpu.py runs the same files through the host routes."""
import pytest

import hast_amd
from tests.gz_crafted_corpus import LENIENT, MUST_FAIL, VALID, far_for_a_ring
from tests.test_gz_gpu import ctx  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

# (chunk bytes, chunks per pass, symbols of room per compressed byte, bytes per read)
CONFIGS = ((0, 0, 0.0, 1 << 22), (256, 5, 40, 65537), (64, 1000, 100, 1 << 22), (700, 50, 1.0, 977), (4096, 3, 12, 4099))


def inflate(ctx, path, chunk=0, seg=0, room=0.0, piece=1 << 22):
    with hast_amd.GzReader(ctx, str(path), chunk, seg, room) as z:
        got = z.read_all(piece)
        return got, z.stats()


@pytest.mark.parametrize("name", sorted(VALID))
def test_valid_streams_give_zlibs_bytes(ctx, tmp_path, name):
    blob, want = VALID[name]                                            # (want == zlib's inflate of blob: asserted by the corpus)
    p = tmp_path / (name + ".gz")
    p.write_bytes(blob)
    for chunk, seg, room, piece in CONFIGS:
        got, st = inflate(ctx, p, chunk, seg, room, piece)
        assert got == want, (name, chunk, seg, room, len(got), len(want))
        assert st["out_bytes"] == len(want) and st["compressed_bytes"] == len(blob)
        if name == "far_small_blocks" and chunk == 256:
            print("accepted", st["accepted"])
            assert st["accepted"] >= 130, st                            # more than two groups of 64 through k_gz_maps / k_gz_carry


@pytest.mark.parametrize("ahead", [0, 2])
@pytest.mark.parametrize("name", ["far", "ladder15"])
def test_passes_side_by_side(ctx, tmp_path, monkeypatch, name, ahead):
    monkeypatch.setenv("HAST_GZ_AHEAD", str(ahead))
    blob, want = VALID[name]
    p = tmp_path / (name + ".gz")
    p.write_bytes(blob)
    for chunk, seg, room in ((256, 5, 40), (4096, 3, 12)):
        got, st = inflate(ctx, p, chunk, seg, room, 1 << 20)
        assert got == want, (name, ahead, chunk, seg, len(got), len(want))


def test_far_matches_through_the_ring(ctx, tmp_path, monkeypatch):
    """`far`, padded with further far-match blocks until the file goes round a ring of compressed bytes on the device (pieces of 64 KB:
    with passes of 4 chunks of 1 KB the ring is 320 KB, and files beyond 384 KB go round it)"""
    monkeypatch.setenv("HAST_GZ_PIECE_BYTES", "65536")
    monkeypatch.setenv("HAST_GZ_RING_BYTES", "131072")
    blob, want = far_for_a_ring(400_000)
    p = tmp_path / "far_ring.gz"
    p.write_bytes(blob)
    got, st = inflate(ctx, p, 1024, 4, 50, 99_999)
    assert got == want, (len(got), len(want))
    assert st["ring_bytes"] > 0 and st["ring_laps"] >= 1, st


def read_until_error(ctx, path, chunk):
    got = bytearray()
    try:
        with hast_amd.GzReader(ctx, str(path), chunk) as z:
            while True:
                a = z.read(1 << 20)
                if a.size == 0:
                    return bytes(got), None
                got += a.tobytes()
    except hast_amd.HastError as e:
        return bytes(got), e


@pytest.mark.parametrize("name", sorted(MUST_FAIL))
def test_what_zlib_refuses_is_refused(ctx, tmp_path, name):
    blob, prefix = MUST_FAIL[name]
    p = tmp_path / (name + ".gz")
    p.write_bytes(blob)
    for chunk in (0, 256, 4096):
        got, err = read_until_error(ctx, p, chunk)
        assert err is not None, (name, chunk, len(got))
        assert err.status in (8, 9), (name, chunk, err.status)
        assert prefix.startswith(got), (name, chunk, len(got), len(prefix))     # what was delivered in front of the damage is real data


@pytest.mark.parametrize("name", sorted(LENIENT))
def test_lenient_cases_give_an_error_or_the_simulated_bytes(ctx, tmp_path, name):
    blob, want = LENIENT[name]
    p = tmp_path / (name + ".gz")
    p.write_bytes(blob)
    for chunk in (0, 256, 4096):
        got, err = read_until_error(ctx, p, chunk)
        print(name, chunk, "error" if err else "accepted")
        if err is None:
            assert got == want, (name, chunk, len(got), len(want))
        else:
            assert err.status in (8, 9) and want.startswith(got), (name, chunk, err.status)
