"""An independent restatement of stage 03's rows (`classify_read --rows device`, hast_amd/csrc/rr_core.h): the class by
tests/rb_model.py, the density through Python's own "%0.6f" (correctly rounded, ties to even, like glibc's printf), the names from
`rs_corpus.read_file`.  The tests of rr_core.h, of hast_rs_rows_device / hast_rs_next_rows and of the program compare with it."""
import numpy as np

from tests import rb_model as rb
from tests import rs_corpus as rc


def density_text(v, t):
    return b"%0.6f" % (v / t)


def row(name, v0, v1, t0, t1):
    """(the row's bytes, its class); both set sizes at least 1"""
    assert t0 >= 1 and t1 >= 1
    c = rb.read_class(v0, v1, t0, t1)
    if c == 2:
        return name + b"\tambiguous\t0.0\n", c
    return name + b"\thaplotype%d\t" % c + density_text((v0, v1)[c], (t0, t1)[c]) + b"\n", c


def rows(names, votes, t0, t1):
    """(text, [count0, count1, count2], [bytes of row i]) of the reads in order; votes[i] = (v0, v1)"""
    out, count, sizes = [], [0, 0, 0], []
    for name, (v0, v1) in zip(names, votes):
        text, c = row(name, int(v0), int(v1), t0, t1)
        out.append(text)
        count[c] += 1
        sizes.append(len(text))
    return b"".join(out), count, sizes


def file_rows(fmt, data, votes, t0, t1):
    """the rows of a file (the FASTQ tail's record included), or rc.ERR"""
    recs = rc.read_file(fmt, data)
    if recs == rc.ERR:
        return rc.ERR
    return rows([n for n, _ in recs], votes[:len(recs)], t0, t1)


def splitmix64_pairs(n, seed):
    """the (v, t) arrays of tests/native/test_rr_core.cpp's `rand N SEED`: splitmix64, low word v, high word t, 0 made 1"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9e3779b97f4a7c15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
        z ^= z >> np.uint64(31)
    v, t = z & np.uint64(0xffffffff), z >> np.uint64(32)
    return np.maximum(v, 1), np.maximum(t, 1)


def density_lines(v, t):
    """b"%0.6f\\n" of v / t for arrays of integers below 2^53 (the division is IEEE's, as in C), joined"""
    d = (np.asarray(v, dtype=np.float64) / np.asarray(t, dtype=np.float64)).tolist()
    step = 20000
    return b"".join((b"%0.6f\n" * len(d[i:i + step])) % tuple(d[i:i + step]) for i in range(0, len(d), step))
