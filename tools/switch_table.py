#!/usr/bin/env python3
"""The table of environment switches in INTEGRATION.md, printed from the rows of hast_amd/csrc/switches.h.

    tools/switch_table.py            print the section (what stands between the two markers, markers included)
    tools/switch_table.py --write    rewrite the section of INTEGRATION.md in place

tests/test_switches_cpu.py holds the document to what this prints.  Standard library only."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "hast_amd", "csrc", "switches.h")
DOCUMENT = os.path.join(ROOT, "INTEGRATION.md")
BEGIN = "<!-- switches: printed by tools/switch_table.py from hast_amd/csrc/switches.h, not edited by hand -->"
END = "<!-- /switches -->"
STRING = r'"((?:[^"\\]|\\.)*)"'
ROW = re.compile(r"^\s*X\((\w+), (\w+), ([^,]+), ([^,]+), (\w+), %s, %s, %s, %s\)\s*\\?$" % (STRING, STRING, STRING, STRING))
FIELDS = ("name", "kind", "lo", "hi", "policy", "words", "default", "reader", "meaning")


def rows(header=HEADER):
    """the rows of HAST_SWITCHES(X), in order, as dicts; lo and hi as the text of the header (NOLIM: no upper bound)"""
    text = open(header, encoding="utf-8").read()
    body = text[text.index("#define HAST_SWITCHES(X)"):]
    body = body[:body.index("\n\n")]
    out = []
    for line in body.splitlines()[1:]:
        m = ROW.match(line)
        assert m, "switches.h: not a row of the table: %s" % line
        out.append(dict(zip(FIELDS, m.groups())))
    return out


def values(r):
    span = "%s or more" % r["lo"] if r["hi"] == "NOLIM" else "%s to %s" % (r["lo"], r["hi"])
    outside = "clamped" if r["policy"] == "Clamp" else "ignored"
    return {"Flag": "flag", "FlagDefaultOn": "flag, on by default",
            "Int": "integer, %s (outside: %s)" % (span, outside),
            "Size": "count, %s (outside: %s)" % (span, outside),
            "Real": "number, %s (outside: %s)" % (span, outside),
            "Word": ", ".join("`%s`" % w for w in r["words"].split("|"))}[r["kind"]]


def section():
    lines = [BEGIN,
             "Every environment variable the library and the programs read, with one grammar per kind (`hast_amd/csrc/switches.h`).  A *flag* is on",
             "when the variable is set to anything but the empty string and `0`; a flag that is *on by default* goes off for exactly `0`.  An *integer*",
             "and a *number* must parse as a whole; a *count* is decimal digits with at most one of `K`, `M`, `G` behind them (2^10, 2^20, 2^30, either",
             "case).  A value that is not what the row takes -- trailing bytes, an unknown word, a number outside a range that says *ignored* -- counts",
             "as unset, and one line on stderr says so: `hast: <variable>=<text> is not <what the row takes>; ignored`.  Each is read when the column",
             "says, not before and not again.  The aliases of `classify`'s flags are explained with their flags below.",
             "",
             "| variable | values | default | read by, when | meaning |",
             "|---|---|---|---|---|"]
    for r in rows():
        cells = ["`%s`" % r["name"], values(r), r["default"], r["reader"], r["meaning"]]
        assert not any("|" in c for c in cells), r["name"]
        lines.append("| " + " | ".join(cells) + " |")
    lines.append(END)
    return "\n".join(lines) + "\n"


def in_document(text):
    """(start, end) of the section in the document's text, markers and the newline behind END included"""
    a, b = text.index(BEGIN), text.index(END) + len(END) + 1
    return a, b


def main(argv):
    if argv[1:] == ["--write"]:
        text = open(DOCUMENT, encoding="utf-8").read()
        a, b = in_document(text)
        open(DOCUMENT, "w", encoding="utf-8").write(text[:a] + section() + text[b:])
    elif argv[1:]:
        sys.exit(__doc__)
    else:
        sys.stdout.write(section())


if __name__ == "__main__":
    main(sys.argv)
