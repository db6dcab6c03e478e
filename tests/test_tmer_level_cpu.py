"""The searched t-mer levels inside the open-closed classes, on the host: the 2-KB nibble table k_classify_f keeps in LDS
(tests/native/test_tmer_level.cpp), and the evaluator of the search tool (tools/sim/tmer_rank_search.cpp), which must
reproduce the runs per read tools/sim/tmer_order_sim.cpp measured for the hash order and for open-closed
(profiles/tmer_order_sim.txt: 23.677 and 22.943 at K = 21, 19.737 and 19.182 at config 5's geometry)."""
import json
import os
import subprocess

from tests.conftest import ROOT


def test_tmer_level_table(tmp_path):
    exe = tmp_path / "test_tmer_level"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "test_tmer_level.cpp")], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, (r.stdout.decode()[-500:], r.stderr.decode()[-2000:])
    assert r.stdout.startswith(b"ok ")


def test_rank_search_evaluator(tmp_path):
    exe = tmp_path / "tmer_rank_search"
    subprocess.run(["g++", "-O2", "-std=c++20", "-pthread", "-o", str(exe),
                    os.path.join(ROOT, "tools", "sim", "tmer_rank_search.cpp")], check=True)
    r = subprocess.run([str(exe), "--eval-only", "--test", "8"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = {d["order"]: d for d in (json.loads(x) for x in r.stdout.decode().splitlines() if x.startswith("{"))}
    for order, c3, c5 in (("hash", 23.677, 19.737), ("oc", 22.943, 19.182)):
        assert abs(got[order]["runs_per_read_c3"] - c3) < 0.06, got[order]
        assert abs(got[order]["runs_per_read_c5"] - c5) < 0.06, got[order]
    # the table in the tree: what its header records, and better than open-closed in both geometries
    assert got["table"]["runs_per_read_c3"] < 22.4 and got["table"]["runs_per_read_c5"] < got["oc"]["runs_per_read_c5"], got["table"]
