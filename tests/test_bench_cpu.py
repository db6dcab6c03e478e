"""bench.py's host side without a GPU: the --dump-outputs writer (float64 files, a fixed seeded sample of long outputs with
the positions beside it, totals over every position, the 64-MB bound) and the refusal of a run without timed steps."""
import os
import subprocess
import sys

import numpy as np

from tests.conftest import ROOT


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path):
    import bench
    n = 3 * bench.DUMP_SAMPLE + 7
    c = np.random.default_rng(3).integers(0, 1 << 20, size=(3, n), dtype=np.uint64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), columns={"c0": c[0], "c1": c[1], "neg": c[2]}, index_name="barcode")
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["barcode.npy", "c0.npy", "c1.npy", "neg.npy", "totals.npy"] == sorted(os.listdir(tmp_path / "b"))
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in names}
    assert all(x.dtype == np.float64 for x in a.values()) and sum(x.nbytes for x in a.values()) <= 64 << 20
    for f in names:
        assert np.array_equal(a[f[:-4]], np.load(tmp_path / "b" / f)), f           # the same sample every time
    idx = a["barcode"].astype(np.int64)
    assert len(idx) == bench.DUMP_SAMPLE and np.all(np.diff(idx) > 0) and idx[-1] < n
    for j, k in enumerate(("c0", "c1", "neg")):
        assert np.array_equal(a[k], c[j][idx].astype(np.float64))
    assert list(a["totals"]) == [float(x.sum()) for x in c]


def test_a_run_needs_timed_steps():
    r = subprocess.run([sys.executable, "bench.py", "--steps", "0"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 2 and b"--steps" in r.stderr and not r.stdout
