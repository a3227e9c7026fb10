#!/usr/bin/env python3
"""Writes tests/golden/make_windows.json: what the reference's own python/makeWindows.py (split_and_merge) and
python/selectCandidates.py (selectCandidates) write for the inputs below.  These ARE reference outputs.  Run only where the reference
tree is present (oracle/Makefile names it; REFERENCE=<dir> overrides), like make_hapalign_fixtures.py:

    python tests/golden/make_windows_fixtures.py

The two scripts are Python 2.  They are loaded IN MEMORY: lib2to3's RefactoringTool.refactor_string translates the text and the result
is exec'd into a module object; nothing of their text, translated or not, is written anywhere.  One substitution is made, on the
translated text of makeWindows.py: `numVar/int(maxVarPerWindow)` becomes `numVar//int(maxVarPerWindow)` — Python 2's meaning of that
line (python/makeWindows.py:90; under Python 3 the true division hands range() a float at python/makeWindows.py:95).  The mean of
python/makeWindows.py:117 goes to stderr only and is not stored.

Stored per case: the input lines, the options, and either the files the script wrote ({"N": [lines]} by the number in PREFIX.N.txt)
or the error it raised.  Python 3's dict keeps insertion order, so targets come in order of first appearance — the order
host/windows.hpp defines — and file numbering and line order compare directly.  The order of the tokens INSIDE a line is the walk of a
Python set of tuples (python/makeWindows.py:64) and means nothing: a comparison must take each line's bounds and number of tokens
exactly and its tokens as a sorted list — taken over the lines of one cluster where a cluster of more than 16 tokens continues on
further lines, since the same walk decides which 16 share a line."""
import contextlib
import glob
import io
import json
import os
import re
import sys
import tempfile
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "make_windows.json")


def reference_dir():
    if os.environ.get("REFERENCE"):
        return os.environ["REFERENCE"]
    return re.search(r"^REFERENCE \?= *(\S+)", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M).group(1)


def load(name, substitutions=()):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from lib2to3 import refactor
        tool = refactor.RefactoringTool(refactor.get_fixers_from_package("lib2to3.fixes"))
        text = open(os.path.join(reference_dir(), "python", name + ".py")).read()
        text = str(tool.refactor_string(text, name))
    for old, new in substitutions:
        assert text.count(old) == 1, (name, old)
        text = text.replace(old, new)
    mod = types.ModuleType(name)
    exec(compile(text, name, "exec"), mod.__dict__)
    return mod


def cluster_line(tid, pos, n, start=0):
    """one input line with n distinct deletions at pos"""
    alphabet = "ACGT"
    seqs = []
    for k in range(start, start + n):
        seqs.append("".join(alphabet[(k >> (2 * j)) & 3] for j in range(4)))
    return "%s %d %s # %s" % (tid, pos, " ".join("-" + s for s in seqs), " ".join("1" for _ in seqs))


WINDOW_CASES = [
    # gaps of exactly minDist and minDist + 1
    dict(name="gap_minDist_and_plus_one", minDist=20, n=1000, lines=["chr1 1000 -AC # 3", "chr1 1020 +G # 2", "chr1 1041 -T # 1", "chr1 1062 -TT # 1"]),
    # a chain of three links (each gap <= minDist, the ends 45 apart)
    dict(name="chain_of_three_links", minDist=20, n=1000, lines=["chr1 500 -A # 1", "chr1 515 +CA # 1", "chr1 530 -GG # 1", "chr1 545 +T # 1", "chr1 600 -C # 1"]),
    # two targets: the second one's first file continues the numbering; a numeric target > 24 and target 0 (the warning)
    dict(name="two_targets", minDist=20, n=1000, lines=["chr2 100 -A # 1", "chr2 300 -C # 1", "chr1 200 +GT # 4", "chr2 310 +A # 1", "25 77 -A # 1", "0 90 +C # 1"]),
    # the left clamp, and maxRef starting at 0
    dict(name="left_clamp", minDist=20, n=1000, lines=["chr1 30 -ACG # 2", "chr1 200 -A # 1"]),
    dict(name="lone_insertion_at_5", minDist=20, n=1000, lines=["chr1 5 +AC # 2"]),
    dict(name="lone_insertion_at_0", minDist=20, n=1000, lines=["chr1 0 +A # 2"]),
    # a SNP token beside indels, and alone
    dict(name="snp_token", minDist=20, n=1000, lines=["chr1 700 A=>C -AC # 1 1", "chr1 900 G=>T # 1"]),
    # 16, 17, 32 and 33 variants in one cluster
    dict(name="cluster_of_16", minDist=20, n=1000, lines=[cluster_line("chr1", 1000, 16)]),
    dict(name="cluster_of_17", minDist=20, n=1000, lines=[cluster_line("chr1", 1000, 10), cluster_line("chr1", 1004, 7, 10)]),
    dict(name="cluster_of_32", minDist=20, n=1000, lines=[cluster_line("chr1", 1000, 20), cluster_line("chr1", 1010, 12, 20), "chr1 5000 -A # 1"]),
    dict(name="cluster_of_33", minDist=20, n=1000, lines=[cluster_line("chr1", 1000, 33)]),
    # a duplicate (pos, variant): on one line, and on two lines of the same position
    dict(name="duplicate_pair", minDist=20, n=1000, lines=["chr1 100 -AC -AC +G # 1 1 1", "chr1 100 +G -T # 1 1", "chr1 105 -AC # 1"]),
    # numWindowsPerFile = 1 and 3: a file holds n + 2 clusters
    dict(name="files_of_1", minDist=20, n=1, lines=["chr1 %d -A # 1" % (1000 * k) for k in range(1, 9)] + ["chr2 %d +C # 1" % (1000 * k) for k in range(1, 5)]),
    dict(name="files_of_3", minDist=20, n=3, lines=["chr1 %d -A # 1" % (1000 * k) for k in range(1, 13)] + ["chr2 50 +C # 1"]),
    # a 17-variant cluster counts once towards the file's clusters
    dict(name="files_count_clusters_not_lines", minDist=20, n=1, lines=[cluster_line("chr1", 100, 17), "chr1 1000 -A # 1", "chr1 2000 -A # 1", "chr1 3000 -A # 1"]),
    # minDist = 0: nothing joins (distinct positions are at least 1 apart)
    dict(name="minDist_0", minDist=0, n=1000, lines=["chr1 100 -A # 1", "chr1 101 -C # 1", "chr1 101 +G # 1", "chr1 103 -T # 1"]),
    # unsorted input, lines without counts, a large minDist
    dict(name="unsorted_no_counts", minDist=45, n=1000, lines=["chr1 900 -A", "chr1 100 +CC", "chr1 940 -G", "chr1 145 -T", "chr1 191 -AA"]),
    # the errors
    dict(name="unrecognized_variant", minDist=20, n=1000, lines=["chr1 100 -A # 1", "chr1 200 ACG # 1"]),
    dict(name="variant_too_short", minDist=20, n=1000, lines=["chr1 100 - # 1"]),
]

FILTER_CASES = [
    # default bounds (2 / 10000000): counts summed over consecutive lines of a position, per variant string
    dict(name="default_bounds", minCount=2, maxCount=10000000,
         lines=["chr1 100 -A +C # 1 2", "chr1 100 -A # 1", "chr1 150 -G # 1", "chr1 160 +T -CC # 5 1", "chr1 160 -CC # 1", "chr1 400 -A # 7"]),
    dict(name="minCount_1", minCount=1, maxCount=10000000,
         lines=["chr1 100 -A +C # 1 2", "chr1 100 -A # 1", "chr1 150 -G # 1", "chr1 160 +T -CC # 5 1", "chr1 160 -CC # 1", "chr1 400 -A # 7"]),
    dict(name="maxCount_4", minCount=2, maxCount=4, lines=["chr1 100 -A +C # 1 2", "chr1 100 -A # 4", "chr1 150 -G # 4", "chr1 160 +T # 2"]),
    # two targets: the buffer is not emptied when the target changes, so chr1's last position never comes out
    dict(name="two_targets", minCount=1, maxCount=10000000, lines=["chr1 100 -A # 2", "chr1 200 -C # 2", "chr2 50 +G # 3", "chr2 60 -T # 1"]),
    # the two errors
    dict(name="target_comes_back", minCount=2, maxCount=10000000, lines=["chr1 100 -A # 2", "chr2 50 +G # 3", "chr1 300 -C # 2"]),
    dict(name="position_goes_down", minCount=2, maxCount=10000000, lines=["chr1 100 -A # 2", "chr1 90 +G # 3"]),
]


def main():
    make_windows = load("makeWindows", [("numVar/int(maxVarPerWindow)", "numVar//int(maxVarPerWindow)")])
    select = load("selectCandidates")
    out = dict(windows=[], filter=[])
    sink = io.StringIO()
    for c in WINDOW_CASES:
        with tempfile.TemporaryDirectory() as d:
            inp, prefix = os.path.join(d, "in.txt"), os.path.join(d, "w")
            open(inp, "w").write("".join(l + "\n" for l in c["lines"]))
            rec = dict(c)
            try:
                with contextlib.redirect_stderr(sink), contextlib.redirect_stdout(sink):
                    make_windows.split_and_merge(inputVarFile=inp, windowFilePrefix=prefix, minDist=c["minDist"], variantsPerFile=c["n"])
            except NameError as e:
                rec["error"] = str(e)
            else:
                rec["files"] = {re.search(r"\.(\d+)\.txt$", f).group(1): open(f).read().split("\n")[:-1] for f in glob.glob(prefix + ".*.txt")}
            out["windows"].append(rec)
    for c in FILTER_CASES:
        with tempfile.TemporaryDirectory() as d:
            inp, outp = os.path.join(d, "in.txt"), os.path.join(d, "out.txt")
            open(inp, "w").write("".join(l + "\n" for l in c["lines"]))
            rec = dict(c)
            try:
                with contextlib.redirect_stderr(sink), contextlib.redirect_stdout(sink):
                    select.selectCandidates(inputFile=inp, outputFile=outp, parameters=dict(minCount=c["minCount"], maxCount=c["maxCount"]))
            except NameError as e:
                rec["error"] = str(e)
            else:
                rec["selected"] = open(outp).read().split("\n")[:-1]
            out["filter"].append(rec)
    json.dump(out, open(OUT, "w"), indent=0, sort_keys=True)
    print("wrote %s: %d window cases, %d filter cases" % (OUT, len(out["windows"]), len(out["filter"])))


if __name__ == "__main__":
    sys.exit(main())
