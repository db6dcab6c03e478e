"""An independent restatement of the read bins of `classify_read --bin-reads` (hast_amd/csrc/rb_core.h): the extents of a file's
records taken from its lines, the way `rs_corpus.read_file` restates the reference's reader (not in terms of a newline index), and
the class of a read from its two votes.  The tests of rb_host.h, of hast_rs_next_binned and of the program compare with it."""
from tests import rs_corpus as rc

CLASSES = ("haplotype0", "haplotype1", "ambiguous")


def density(v, t):
    """(double)v / t as IEEE does it: inf for v > 0 over 0, NaN for 0 over 0 (Python's true division is correctly rounded too)"""
    if t == 0:
        return float("inf") if v > 0 else float("nan")
    return v / t


def read_class(v0, v1, t0, t1):
    d0, d1 = density(v0, t0), density(v1, t1)
    if not d0 > 0 and not d1 > 0:
        return 2
    return 1 if d1 > d0 else 0


def extents(fmt, data):
    """the bytes of every record of the file, in the order of `rs_corpus.read_file`: FASTQ: four terminated lines as they lie, and the
    file's end, if its header line is terminated, with a newline added unless it ends in one; FASTA: a header line and every terminated
    line up to the next header line, blank ones included; lines in front of the first header and an unterminated last line: nobody's"""
    lines = data.split(b"\n")
    rest = lines.pop()
    out = []
    if fmt == rc.FASTQ:
        whole = len(lines) // 4
        for i in range(whole):
            out.append(b"".join(l + b"\n" for l in lines[4 * i:4 * i + 4]))
        if len(lines) % 4:
            out.append(b"".join(l + b"\n" for l in lines[4 * whole:]) + (rest + b"\n" if rest else b""))
        return out
    cur = None
    for line in lines:
        if line[:1] == b">":
            cur = bytearray()
            out.append(cur)
        if cur is not None:
            cur += line + b"\n"
    return [bytes(e) for e in out]


def runs_by_class(fmt, data, classes):
    """([run0, run1, run2], [count0, count1, count2]) of the file; classes[i]: the class of record i of `read_file`"""
    ext = extents(fmt, data)
    assert len(ext) == len(classes), (len(ext), len(classes))
    out, count = [bytearray(), bytearray(), bytearray()], [0, 0, 0]
    for e, c in zip(ext, classes):
        out[c] += e
        count[c] += 1
    return [bytes(r) for r in out], count


def runs(fmt, data, votes, t0, t1):
    """([run0, run1, run2], [count0, count1, count2], classes) of the file; votes[i] = (v0, v1) of record i of `read_file`"""
    classes = [read_class(int(v0), int(v1), t0, t1) for v0, v1 in votes]
    out, count = runs_by_class(fmt, data, classes)
    return out, count, classes
