"""Inputs for the tests of the stage-00 device ingest of FASTA (sq_core.h namespace sqfa, hast_sq_frame_fasta_device, hast_sq_feed_*):
FASTA as jellyfish reads it -- any line width and line break, records without a sequence, blank lines, '@' and '+' lines, no final
newline, two files that are one stream -- and the builders of the host model and of the host parser's driver."""
import os
import random
import subprocess

from tests.conftest import ROOT

WIDTHS = (1, 7, 59, 60, 61, 150, 4097)
BREAKS = (b"\n", b"\r\n", b"\r\r\n")
COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 1000)
BASES = b"ACGTACGTacgtN"
BLOCKS = (64, 100, 700, 4096, 65536, 1 << 24)


def fasta(seed, n_records, width, brk, max_lines=40, last_newline=True, plain=False):
    """n_records records of `width`-column lines; record i has 1 .. max_lines sequence lines, the last one shorter.  Unless plain: every
    fifth record has no sequence at all (header after header), every seventh header is a lone '>', and blank lines, '@...' and '+' lines
    lie between the sequence lines of some records.  Headers stay under 16 bytes."""
    rng = random.Random(seed)
    out = bytearray()
    for i in range(n_records):
        lone = not plain and i % 7 == 3
        out += (b">" if lone else b">r%d" % i if i % 2 else b">r%d x=%d" % (i, i % 9)) + brk
        if not plain and i % 5 == 4:
            continue
        n_lines = 1 + (i * 7 + seed) % max_lines
        for l in range(n_lines):
            w = width if l + 1 < n_lines else 1 + rng.randrange(width)
            out += bytes(rng.choice(BASES) for _ in range(w)) + brk
            if not plain and (i + l) % 11 == 5:
                out += (brk, b"@r1" [:width] + brk, b"+" + brk, brk + brk)[(i + l) % 4]
    if not last_newline:
        del out[len(out) - len(brk):]
    return bytes(out)


def longest_line(files):
    """the longest line of the stream, its line break included"""
    return max(len(l) + 1 for l in b"".join(files).split(b"\n"))


def corpus():
    """(name, files, longest line): `files` are read one after the other as ONE input"""
    out = []

    def add(name, *files):
        out.append((name, list(files), longest_line(files)))
    for b, brk in enumerate(BREAKS):
        for width in WIDTHS:
            big = width >= 150
            add("w%d_b%d" % (width, b), fasta(3 * width + b, 5 if big else 9, width, brk, max_lines=3 if width > 150 else 40))
            add("w%d_b%d_nonl" % (width, b), fasta(5 * width + b, 3, width, brk, max_lines=2 if big else 5, last_newline=False))
        for n in COUNTS:
            for last in (True, False):
                add("n%d_b%d_%s" % (n, b, "nl" if last else "nonl"), fasta(7 * n + b, n, 7, brk, max_lines=5 if n < 1000 else 3, last_newline=last))
        add("plain60_b%d" % b, fasta(11 + b, 65, 60, brk, max_lines=4, plain=True))
        add("hdr_only_b%d" % b, b">a" + brk + b">b" + brk + b">" + brk)
        add("no_header_line_b%d" % b, b">" + brk + b"ACGTNacgt" + brk + b"@x" + brk + b"+" + brk + b"!!ac")
        whole = fasta(13 + b, 17, 7, brk)
        cut = len(whole) // 2
        while whole[cut - 1:cut] in (b"\n", b"\r") or whole[cut:cut + 1] in (b"\n", b"\r"):      # inside a line
            cut += 1
        add("two_files_b%d" % b, whole[:cut], whole[cut:])
    rng = random.Random(40)
    add("lines_1_to_40", b"".join(b">s%d\n" % n + b"".join(bytes(rng.choice(BASES) for _ in range(7)) + b"\n" for _ in range(n)) for n in range(1, 41)))
    add("issue_example", b">a\r\nAC\r\r\n\r\nGT\n>\n>b x\n@r1\n+\nNNac")
    add("issue_two_files", b">a\nACG\n", b">b\nTTT")
    add("only_header_nonl", b">only")
    add("lone_gt", b">")
    add("lone_gt_nl", b">\n")
    add("gt_and_blank_lines", b">\n\n\r\n\n")
    add("one_base", b">\nA")
    return out


def write_case(directory, name, files):
    paths = []
    for i, data in enumerate(files):
        p = os.path.join(str(directory), "%s.%d.fa" % (name, i))
        with open(p, "wb") as f:
            f.write(data)
        paths.append(p)
    return paths


def build_model(out_dir, sanitize=False, shared=False):
    """tests/native/test_sq_fasta.cpp as a program (optionally under ASan + UBSan) or, shared=True, as the model's library"""
    src = os.path.join(ROOT, "tests", "native", "test_sq_fasta.cpp")
    if shared:
        out = os.path.join(str(out_dir), "libsq_fasta_model.so")
        cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DSQ_FASTA_MODEL_LIB", "-o", out, src]
    else:
        out = os.path.join(str(out_dir), "test_sq_fasta_san" if sanitize else "test_sq_fasta")
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra"] + (["-fsanitize=address,undefined"] if sanitize else []) + ["-o", out, src]
    subprocess.run(cmd, check=True)
    return out


def build_parser_driver(out_dir):
    out = os.path.join(str(out_dir), "test_seqstream")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", out, os.path.join(ROOT, "tests", "native", "test_seqstream.cpp")], check=True)
    return out


def parser_stream(driver, paths):
    """what SeqParser hands its sink for the files read as one input"""
    return subprocess.run([driver, "-c"] + list(paths), stdout=subprocess.PIPE, check=True).stdout


def header_count(files):
    """the records of an input, counted without any parser: its lines that start with '>'"""
    return sum(1 for l in b"".join(files).split(b"\n") if l.rstrip(b"\r")[:1] == b">")
