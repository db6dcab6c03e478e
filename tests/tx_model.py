"""A short restatement of fake_10x.pl (stage 02: stLFR pairs -> 10x FASTQ), the rules of hast_amd/csrc/tx_core.h in Python.
The goldens under tests/golden/fake10x/ hold it (and the C host model) to what the script itself wrote."""
import gzip
import os
import re

_LINE = re.compile(rb"[^\n]*\n|[^\n]+")
GOLDEN_ARGS = ("r1.fq.gz", "r2.fq.gz", "map.txt")        # the names the goldens' stdout was recorded with


# maps the device path cannot take: edge's map and one more line.  The script's reads are edge's; its outputs are edge's too
# unless the line adds a key some header has (the generator checks that), so only fb_emptykey has files of its own
FALLBACK = {"fb_value17": (b"LONGV\tAAAAAAAAAAAAAAAAA\n", "value longer than 16 bytes"), "fb_key16": (b"K234567890123456\tACGT\n", "key longer than 15 bytes"),
            "fb_emptykey": (b"\tGGGG\n", "empty key")}


def golden(case, name):
    """a file of tests/golden/fake10x/<case>; the larger ones are kept gzipped, the fallback cases borrow from edge (above)"""
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fake10x")
    if case in FALLBACK and name == "map.txt":
        return golden("edge", name) + FALLBACK[case][0]
    if case in FALLBACK and (name in ("r1.fq", "r2.fq") or not os.path.isdir(os.path.join(d, case))):
        case = "edge"
    p = os.path.join(d, case, name)
    return open(p, "rb").read() if os.path.exists(p) else gzip.open(p + ".gz").read()


def banner(a1, a2, a3):
    return ("Merge stLFR reads into 10X format !\n read1 :  %s \n. read2 : %s \n map file : %s\n" % (a1, a2, a3)).encode()


def parse_map(text):
    """chomp, split at tabs, map[field 0] = field 1; a later line wins; no tab: the empty string"""
    m = {}
    for line in _LINE.findall(text):
        f = line.rstrip(b"\n").split(b"\t")
        m[f[0]] = f[1] if len(f) > 1 else b""
    return m


def device_ok(m):
    """(ok, reason) as hast_tx_map_load reports them"""
    if any(len(k) == 0 for k in m):
        return False, "empty key"
    if any(len(k) > 15 for k in m):
        return False, "key longer than 15 bytes"
    if any(len(v) > 16 for v in m.values()):
        return False, "value longer than 16 bytes"
    return True, "none"


def key_of(header):
    """header: the line without its newline"""
    f0 = header.split(b"\t", 1)[0]
    at = f0.find(b"#")
    if at < 0:
        return b""
    return re.match(rb"[^#/]*", f0[at + 1:]).group(0)


def convert(m, r1, r2, used=0, headers=0):
    """-> (out1, out2, progress + total lines of stdout, used, headers); r1 / r2 are the whole inputs"""
    a, b = iter(_LINE.findall(r1)), iter(_LINE.findall(r2))
    out1, out2, log = [], [], []
    for head in a:
        headers += 1
        if headers % 1000000 == 0:
            log.append(b"process %d (Mb) pair of reads now  \n" % (headers // 1000000))
        value = m.get(key_of(head.rstrip(b"\n") if head.endswith(b"\n") else head))
        if value is None:
            for _ in range(3):
                next(a, None)
            for _ in range(4):
                next(b, None)
            continue
        used += 1
        name = b"@ST-E0:0:SIMULATE:8:0:0:%d" % used
        out1 += [name, b" 1:N:0:NAAGTGCT\n", value, b"ATCGAGN", next(a, b""), next(a, b""), b"F" * 22 + b"#", next(a, b"").replace(b"!", b"#")]
        next(b, None)
        out2 += [name, b" 2:N:0:NAAGTGCT\n", next(b, b""), next(b, b""), next(b, b"").replace(b"!", b"#")]
    log.append(b"Total %d pair reads and used %d pairs.\n" % (headers, used))
    return b"".join(out1), b"".join(out2), b"".join(log), used, headers
