"""The output table of `classify` and the three barcode lists of --phase-reads, restated independently of hast_amd/csrc/rows_core.h:
the order is sorted() on bytes, the call uses Python floats (IEEE doubles) in the reference's sequence of operations (classify.cpp:66-86),
the rows are formatted with %d."""
INT_MAX = 2 ** 31 - 1


def hap(text, c0, c1, n0, n1, w0, w1):
    if text in (b"0_0_0", b"0_0", b"0"):
        return -1
    if c0 > 0 and c1 > 0:
        df0 = float(c0) / float(n0)
        df1 = float(c1) / float(n1)
        df0 *= w0
        df1 *= w1
        if df0 > df1:
            return 0
        if df1 > df0:
            return 1
        return -1
    if c0 > 0:
        return 0
    if c1 > 0:
        return 1
    return -1


def list_of(h):
    return {0: 1, 1: 2, -1: 3}[h]


class Tables:
    pass


def build(names, c0, c1, n0, n1, w0, w1):
    """names: distinct bytes of at most 15 bytes each, by id; c0, c1: ints by id"""
    assert len(set(names)) == len(names) and all(len(t) <= 15 for t in names)
    t = Tables()
    haps = [hap(names[i], c0[i], c1[i], n0, n1, w0, w1) for i in range(len(names))]
    t.cls = [list_of(h) for h in haps]
    t.order = sorted(range(len(names)), key=lambda i: names[i])
    t.table = b"".join(names[i] + b"\t%d\t%d\t%d\n" % (haps[i], c0[i], c1[i]) for i in t.order)
    t.lists = [b"".join(names[i] + b"\n" for i in t.order if t.cls[i] == l) for l in (1, 2, 3)]
    t.any_sep = any(b"#" in x or b"/" in x for x in names)
    t.past_int = any(a > INT_MAX or b > INT_MAX for a, b in zip(c0, c1))
    return t
