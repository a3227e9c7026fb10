#!/usr/bin/env python3
"""Writes tests/golden/reference_line_counts.json: the number of lines of every file of the reference tree that
tests/test_citations.py can see cited (top-level files, python/*, and python/utils/* under their bare names when no top-level
file has that name).  Counts only: no reference text is stored.

    python tests/golden/make_reference_line_counts.py REFERENCE_TREE"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def count(path):
    return sum(1 for _ in open(path, errors="ignore"))


def line_counts(ref):
    nlines = {}
    for f in os.listdir(ref):
        if os.path.isfile(os.path.join(ref, f)):
            nlines[f] = count(os.path.join(ref, f))
    pydir = os.path.join(ref, "python")
    for f in os.listdir(pydir) if os.path.isdir(pydir) else []:
        if os.path.isfile(os.path.join(pydir, f)):
            nlines["python/" + f] = count(os.path.join(pydir, f))
    utils = os.path.join(pydir, "utils")
    for f in os.listdir(utils) if os.path.isdir(utils) else []:      # python/utils/Fasta.py is cited as "Fasta.py:…" / "python/utils/Fasta.py:…"
        if os.path.isfile(os.path.join(utils, f)) and f not in nlines:
            nlines[f] = count(os.path.join(utils, f))
    return nlines


if __name__ == "__main__":
    nlines = line_counts(sys.argv[1])
    json.dump(dict(note="line counts of the reference tree's files (tests/test_citations.py)", nlines=dict(sorted(nlines.items()))),
              open(os.path.join(HERE, "reference_line_counts.json"), "w"), indent=0)
    print(len(nlines), "files")
