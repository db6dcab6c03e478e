"""bench.py on one GPU (-m gpu): a plain run prints the headline line, --full adds the per-kernel clock and the roofline over
the SAME computation, and --dump-outputs writes what the timed path returned (equal from run to run with the same arguments)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
C1 = ["--workload", "c1", "--batch-reads", "300000", "--batches-per-step", "1", "--cpu-seconds", "0"]
C5 = ["--workload", "c5", "--keys-per-hap", "1000000", "--read-len", "6000", "--batch-reads", "3000", "--cpu-seconds", "0", "--batches-per-step", "1"]


def _run(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, "bench.py"] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = r.stdout.decode().strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def _load(d):
    out = {}
    for f in sorted(os.listdir(d)):
        assert f.endswith(".npy"), f
        out[f[:-4]] = np.load(os.path.join(d, f))
        assert out[f[:-4]].dtype == np.float64, f
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    return out


def test_plain_line_and_outputs_equal_full(tmp_path):
    plain = _run(["--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "plain")] + C1)
    full = _run(["--steps", "3", "--warmup", "1", "--full", "--dump-outputs", str(tmp_path / "full")] + C1)
    for r in (plain, full):
        assert all(k in r for k in HEADLINE) and r["unit"] == "bp/s" and r["higher_is_better"] is True and r["dtype"] == "u64"
        assert r["steps"] == 3 and r["config"]["reads_total"] == 3 * 300000 and r["ms_per_step"] > 0
        assert r["value"] == pytest.approx(3 * 300000 * 150 / (r["ms_per_step"] * 3 / 1e3), rel=1e-9)
    assert "roofline" not in plain and "kernel_ms_avg" not in plain["ranks"]
    assert full["roofline"]["kernel_ms_avg"] > 0 and full["ranks"]["kernel_ms_avg"]["min"] > 0
    assert plain["hits"] == full["hits"] and plain["hits"]["c0"] > 0
    a, b = _load(tmp_path / "plain"), _load(tmp_path / "full")
    assert sorted(a) == ["barcode", "c0", "c1", "neg", "totals"]
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["barcode"], np.arange(plain["config"]["barcodes"]))       # 10k barcodes: every one
    assert list(a["totals"]) == [plain["hits"]["c0"], plain["hits"]["c1"], plain["hits"]["neg_reads"]]
    assert [a["c0"].sum(), a["c1"].sum(), a["neg"].sum()] == list(a["totals"])


def test_dump_outputs_per_read_and_s00(tmp_path):
    r = _run(["--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "c5")] + C5)
    o = _load(tmp_path / "c5")
    assert sorted(o) == ["perread", "read", "totals"]
    assert o["perread"].shape == (3000, 2) and np.array_equal(o["read"], np.arange(3000))
    assert list(o["totals"]) == [r["hits"]["c0"], r["hits"]["c1"]]
    assert list(o["perread"].sum(axis=0)) == [r["hits"]["last_launch_rank0"]["c0"], r["hits"]["last_launch_rank0"]["c1"]]
    s = _run(["--workload", "s00", "--genome", "2e6", "--coverage", "4", "--table-gb", "1", "--steps", "2", "--warmup", "1",
              "--dump-outputs", str(tmp_path / "s00")])
    o = _load(tmp_path / "s00")
    assert sorted(o) == ["histo_p0", "histo_p1", "kmers"] and "cpu_baseline" not in s and s["steps"] == 2
    assert list(o["kmers"]) == s["kmers"]["counted"] + s["kmers"]["distinct"] + [s["kmers"]["union"]]
    assert o["histo_p0"].sum() > 0 and o["histo_p1"].sum() > 0
