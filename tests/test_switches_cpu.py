"""The environment switches: hast_amd/csrc/switches.h is the one table and the one reader, and source, table and document agree.

tests/native/test_switches.cpp runs the reader kind by kind (stand-alone, plain and under ASan + UBSan); the rest is text: no getenv(
outside switches.h, every row read somewhere, INTEGRATION.md's table what tools/switch_table.py prints, no HAST_* word in the
documents, the tools and the tests that is not a row, and the four closed experiments gone."""
import glob
import importlib.util
import os
import re
import subprocess
import sys

import pytest

from tests import kc_geometry_corpus as corpus
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "hast_amd", "csrc")
DELETED = ("HAST_NAME_EARLY", "HAST_COMMIT_IDS", "HAST_GZ_PREALLOC", "HAST_GZ_ARENAS")
# HAST_* words that are variables, and not the C++ code's: what Python reads (the binding, bench.py, the tests themselves), and the
# name tools/gpu uses for "no variable at all"
NOT_THE_TABLES = {"HAST_LIB", "HAST_BENCH_BACKEND", "HAST_BENCH_FORCE_DIST", "HAST_BENCH_SHARE_GPU", "HAST_FUZZ_ITERS", "HAST_FUZZ_SEED", "HAST_HEAVY_FILES",
                  "HAST_HEAVY_ORACLE", "HAST_QUARTERING_EXE", "HAST_UNUSED"}


def load_tool():
    spec = importlib.util.spec_from_file_location("switch_table", os.path.join(ROOT, "tools", "switch_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = load_tool()
ROWS = TOOL.rows()
NAMES = [r["name"] for r in ROWS]


def sources():
    return sorted(p for p in glob.glob(os.path.join(CSRC, "*")) if os.path.isfile(p) and p.endswith((".cpp", ".h", ".hip")))


def read(path):
    return open(path, encoding="utf-8", errors="replace").read()


def build_native(out_dir, sanitize):
    out = os.path.join(str(out_dir), "test_switches_san" if sanitize else "test_switches")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + (["-fsanitize=address,undefined"] if sanitize else []) + \
          ["-o", out, os.path.join(ROOT, "tests", "native", "test_switches.cpp")]
    subprocess.run(cmd, check=True)
    return out


@pytest.mark.parametrize("build", ("plain", "asan_ubsan"))
def test_the_reader_kind_by_kind(tmp_path, build):
    exe = build_native(tmp_path, build == "asan_ubsan")
    err = tmp_path / "stderr.txt"
    env = dict(os.environ, HAST_GZ_TRACE="1", HAST_INFLATE="zlib")            # (the program clears what it finds of the table)
    r = subprocess.run([exe, str(err)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
    said = err.read_bytes()
    assert r.returncode == 0 and r.stderr == b"", (r.stdout.decode()[-3000:], r.stderr.decode()[-2000:], said.decode()[-2000:])
    assert b"runtime error" not in said and b"Sanitizer" not in said, said.decode()[-3000:]
    m = re.fullmatch(r"checks (\d+) failed 0 rows (\d+)\n", r.stdout.decode())
    assert m and int(m.group(1)) > 400 and int(m.group(2)) == len(ROWS), r.stdout
    lines = said.decode().splitlines()
    assert lines and all(re.fullmatch(r"hast: HAST_[A-Z0-9_]+=.* is not .*; ignored", x) for x in lines), lines
    assert len({x.split("=")[0] for x in lines}) == len(lines), "a variable was reported twice"


def test_getenv_is_in_switches_h_alone():
    with_getenv = [os.path.basename(p) for p in sources() if "getenv(" in read(p)]
    assert with_getenv == ["switches.h"], with_getenv


def test_every_row_is_read_somewhere():
    assert len(set(NAMES)) == len(NAMES) and all(re.fullmatch(r"HAST_[A-Z0-9_]+", n) for n in NAMES)
    others = "\n".join(read(p) for p in sources() if os.path.basename(p) != "switches.h")
    unread = [n for n in NAMES if not re.search(r"\bsw::%s\b" % n, others)]
    assert not unread, "rows of switches.h that no other file reads: %s" % unread
    # and nothing reads the environment by a string of its own
    assert not re.findall(r'"HAST_[A-Z0-9_]+"', re.sub(r'setenv\("HAST_[A-Z0-9_]+"', "", others)), "a HAST_ name as a string outside switches.h (other than a setenv)"


def test_the_document_is_what_the_tool_prints():
    text = read(os.path.join(ROOT, "INTEGRATION.md"))
    assert text.count(TOOL.BEGIN) == 1 and text.count(TOOL.END) == 1
    a, b = TOOL.in_document(text)
    assert text[a:b].encode() == TOOL.section().encode()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "switch_table.py")], stdout=subprocess.PIPE, check=True).stdout
    assert out == text[a:b].encode()
    for r in ROWS:
        assert "| `%s` |" % r["name"] in text[a:b]
    assert "`HAST_LIB`" in text[b:]                                            # (the binding's, by hand below the table)


def c_identifiers_of_the_header():
    """HAST_* names include/hast.h defines itself: macros and enumerators, which are no variables"""
    text = read(os.path.join(ROOT, "include", "hast.h"))
    return set(re.findall(r"#\s*(?:define|ifndef)\s+(HAST_[A-Z0-9_]+)", text)) | set(re.findall(r"^\s*(HAST_[A-Z0-9_]+)\s*(?:=[^,]*)?,?\s*(?:/\*.*)?$", text, re.M))


def test_every_switch_the_documents_tools_and_tests_name_is_a_row():
    ids = c_identifiers_of_the_header()
    assert "HAST_OK" in ids and "HAST_NAME_NONE" in ids and not ids & set(NAMES)
    files = [os.path.join(ROOT, "INTEGRATION.md"), os.path.join(ROOT, "README.md"), os.path.join(ROOT, "include", "hast.h")] + \
        sorted(glob.glob(os.path.join(ROOT, "tools", "gpu", "*.sh"))) + sorted(glob.glob(os.path.join(ROOT, "tests", "*.py")))
    assert len(files) > 50
    unknown = {}
    for path in files:
        if os.path.basename(path) == "test_switches_cpu.py":                   # (this file names the deleted ones)
            continue
        for w in set(re.findall(r"HAST_[A-Z0-9_]+", read(path))):
            if w in NAMES or w in NOT_THE_TABLES or w in ids:
                continue
            if w.endswith("_") and any(n.startswith(w) for n in NAMES):        # "HAST_FILTER_*", "HAST_KC_*": a family of rows
                continue
            unknown.setdefault(w, []).append(os.path.relpath(path, ROOT))
    assert not unknown, "HAST_* words that are no row of hast_amd/csrc/switches.h: %s" % unknown


def test_the_closed_experiments_are_gone():
    found = []
    for top in ("hast_amd", "include", "tests", "tools"):
        for d, dirs, names in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [x for x in dirs if x not in ("__pycache__", "golden")]
            for n in names:
                p = os.path.join(d, n)
                if os.path.abspath(p) == os.path.abspath(__file__) or not n.endswith((".cpp", ".h", ".hip", ".py", ".sh", ".md", ".c", ".txt", "Makefile")):
                    continue
                found += [(os.path.relpath(p, ROOT), w) for w in DELETED + ("name_early", "named_early", "launch_fq_name_claim_framed", "ids_from_host =")
                          if w in read(p)]
    assert not found, found
    assert not set(DELETED) & set(NAMES)


def test_the_counter_corpus_clears_every_switch_of_the_count_table():
    of_the_counter = [r["name"] for r in ROWS if r["name"].startswith("HAST_KC_") and r["reader"].startswith("hast_kc")]
    assert len(of_the_counter) >= 7
    assert set(of_the_counter + ["HAST_MINIMIZER"]) <= set(corpus.CLEARED), sorted(set(of_the_counter) - set(corpus.CLEARED))
