#!/usr/bin/env python3
"""Writes tests/golden/hapalign_seqan.json: scores and gapped rows of the SeqAn library that ships with the reference
(<reference>/seqan_library), for the case list below.  These ARE reference outputs.  Run only where the reference tree is present
(oracle/Makefile names it; REFERENCE=<dir> overrides), like make_ref_bits.py:

    python tests/golden/make_hapalign_fixtures.py

The script writes a small driver of its own into a temporary directory, compiles it against the library's headers and keeps only what
it prints.  The driver makes the call DetInDel::alignHaplotypes makes (DInDel.cpp:1436, ObservationModelSeqAn.hpp:324-333): an
Align<DnaString, ArrayGaps> of the reference (row 0) and the haplotype (row 1), globalAlignment with Score<int>(-1, -460, -100, -960).
Stored per case: ref, hap (latin-1 text of the bytes), score, row0, row1."""
import json
import os
import random
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "hapalign_seqan.json")

DRIVER = r"""
#include <iostream>
#include <string>
#include <seqan/align.h>
#include <seqan/graph_align.h>
static std::string unhex(const std::string &h)
{
    std::string s;
    for (size_t i = 0; i + 1 < h.size(); i += 2) s += (char)strtol(h.substr(i, 2).c_str(), 0, 16);
    return s;
}
template <class TRow> static std::string text(const TRow &r, size_t b, size_t e)
{
    std::string s;
    for (size_t p = b; p < e; p++) s += seqan::isGap(r, p) ? '-' : seqan::convert<char>(r[p]);
    return s;
}
int main()
{
    std::string hr, hh;
    seqan::Score<int> score(-1, -460, -100, -960);
    while (std::cin >> hr >> hh) {
        seqan::DnaString ref(unhex(hr)), hap(unhex(hh));
        seqan::Align<seqan::DnaString, seqan::ArrayGaps> align;
        seqan::resize(seqan::rows(align), 2);
        seqan::assignSource(seqan::row(align, 0), ref);
        seqan::assignSource(seqan::row(align, 1), hap);
        int s = seqan::globalAlignment(align, score);
        size_t b = seqan::beginPosition(seqan::cols(align)), e = seqan::endPosition(seqan::cols(align));
        std::cout << s << ' ' << text(seqan::row(align, 0), b, e) << ' ' << text(seqan::row(align, 1), b, e) << std::endl;
    }
    return 0;
}
"""


def reference_dir():
    if os.environ.get("REFERENCE"):
        return os.environ["REFERENCE"]
    return re.search(r"^REFERENCE \?= *(\S+)", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M).group(1)


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def mutate(rng, s, n_sub, n_indel, max_indel):
    s = list(s)
    for _ in range(n_sub):
        if s:
            s[rng.randrange(len(s))] = rng.choice("ACGT")
    for _ in range(n_indel):
        n = rng.randint(1, max_indel)
        p = rng.randrange(len(s) + 1)
        if rng.random() < 0.5:
            s[p:p] = list(rand_seq(rng, n))
        else:
            del s[p:p + n]
    return "".join(s)


def cases():
    """(ref, hap) byte strings: the list of the alignment's test plan.  Deterministic."""
    rng = random.Random(20091)
    out = []

    def add(ref, hap):
        ref = ref.encode("latin-1") if isinstance(ref, str) else bytes(ref)
        hap = hap.encode("latin-1") if isinstance(hap, str) else bytes(hap)
        assert 1 <= len(ref) <= 300 and 1 <= len(hap) <= 300
        out.append((ref, hap))

    # the three examples commented in ObservationModelSeqAn.hpp:278-285
    add("ATGGCGTGACTGATCCTATCCCCGTT", "TTATATGGCGTG")
    add("ATGGCGTGACTGATCCTATCGTCGTT", "CCCGGTGACTCC")
    add("ATGGCGTGACTGATCCTATCGTCGTT", "CTATCGTCTGTAGGTGTCCT")
    # hap = ref
    for n in (1, 2, 7, 64, 65, 130):
        s = rand_seq(rng, n)
        add(s, s)
    # single indels of 1 ... 12 bases, either kind, and two indels (one of each kind, and two of a kind)
    for n in range(1, 13):
        s = rand_seq(rng, 48)
        p = rng.randrange(8, 36)
        add(s, s[:p] + s[p + n:])
        add(s, s[:p] + rand_seq(rng, n) + s[p:])
    for n in range(1, 13):
        s = rand_seq(rng, 70)
        p, q = rng.randrange(8, 24), rng.randrange(40, 56)
        m = rng.randint(1, 12)
        kind = n % 3
        if kind == 0:
            add(s, s[:p] + s[p + n:q] + rand_seq(rng, m) + s[q:])
        elif kind == 1:
            add(s, s[:p] + s[p + n:q] + s[q + m:])
        else:
            add(s, s[:p] + rand_seq(rng, n) + s[p:q] + rand_seq(rng, m) + s[q:])
    # indels inside homopolymers and 2- and 3-mer repeats: one and two periods, both directions, bare and with flanks
    add("ACACACACGT", "ACACACGT")
    add("ACACACGT", "ACACACACGT")
    for a, b in ((8, 10), (10, 8), (1, 3), (3, 1), (5, 6), (6, 5), (20, 21), (64, 66)):
        add("A" * a, "A" * b)
    for unit in ("A", "AC", "ACG"):
        for reps in (4, 9):
            for periods in (1, 2):
                for lf, rf in (("", ""), ("GGTCA", "CTGAT")):
                    long_, short = lf + unit * (reps + periods) + rf, lf + unit * reps + rf
                    add(long_, short)
                    add(short, long_)
    # SNP next to an indel
    s = rand_seq(rng, 40)
    for p in (10, 20, 30):
        flip = {"A": "C", "C": "G", "G": "T", "T": "A"}
        add(s, s[:p] + flip[s[p]] + s[p + 3:])
        add(s, s[:p] + "GA" + flip[s[p]] + s[p + 1:])
        add(s, s[:p - 1] + flip[s[p - 1]] + "TTC" + s[p:])
        add(s, s[:p] + s[p + 2:p + 6] + flip[s[p + 6]] + s[p + 7:])
    # haplotype overhanging the reference at either or both ends, and the other way round
    s = rand_seq(rng, 60)
    for lo, ro in ((4, 0), (0, 5), (3, 6), (1, 1), (12, 0), (0, 12)):
        add(s, rand_seq(rng, lo) + s + rand_seq(rng, ro))
        add(rand_seq(rng, lo) + s + rand_seq(rng, ro), s)
        add(s[lo:], s[:len(s) - ro] if ro else s)
        add(s[:40], rand_seq(rng, lo) + s[:40 - ro])
    # all-mismatch
    for a, b in ((1, 1), (4, 4), (9, 5), (5, 9), (30, 30), (2, 1), (1, 2)):
        add("A" * a, "C" * b)
        add("ACGT" * a, "CATG" * b)
    # N, lower case, U and other bytes (every byte that is no letter of the alphabet is an A)
    add("ACGTNACGTNNACGT", "ACGTAACGTAAACGT")
    add("ACGTAACGTAAACGT", "NCGTNNCGTAANCGN")
    add("acgtacgtacgt", "ACGTACGTACGT")
    add("ACGTACGTACGT", "acgtaCGtacgt")
    add("ACGUACGUuACGT", "ACGTACGTTACGT")
    add("ACGTACGTTACGT", "UCGUACGuUACGU")
    add(b"AC\x00GT\xffCCGTA", b"ACAGTACCGTA")
    add(b"ACAGTACCGTA", b"\x00C\xffGT\x00CCGT\xff")
    add(b"GGRYKMSWGGC", b"GG-*. @[GGC")
    add(b"\x00", b"\xff")
    add(b"TTNNNNTT", b"TTTT")
    add(b"TTTT", b"TTnnXXTT")
    # length 1 on either side
    for one in "ACGT":
        add(one, "ACGT")
        add("ACGT", one)
        add(one, "A")
        add(one, rand_seq(rng, 9))
        add(rand_seq(rng, 9), one)
    # seeded random mutations of random sequences: lengths 1 ... 300, mostly short
    while len(out) < 320:
        k = len(out) % 10
        n = rng.randint(1, 12) if k < 2 else rng.randint(13, 90) if k < 8 else rng.randint(91, 300)
        s = rand_seq(rng, n, "ACGT" if k != 5 else "AC")
        h = mutate(rng, s, rng.randint(0, 3), rng.randint(0, 3), 12)
        if not 1 <= len(h) <= 300:
            h = s
        add(s, h)
    # a deletion and an insertion that touch (a block of seven or more mismatching bases is cheaper as the two gaps): at the start, in the
    # middle and at the end, equal and unequal lengths, next to a SNP, and twice in one alignment.  Which gap comes first is part of the
    # alignment: convertAlignment keys the insertion behind or in front of the deleted bases accordingly.
    R, L = "GTCAGTCAGTTGCA", "ACGTACGTACGGTCA"
    add("A" * 8 + R, "C" * 8 + R)
    add(L + "AGAGAGAGAG" + R, L + "CTCTCTCT" + R)
    add(L + "A" * 8, L + "C" * 8)
    add("A" * 7 + R, "C" * 7 + R)
    add("A" * 6 + R, "C" * 6 + R)                         # six mismatches stay mismatches
    add("AG" * 6 + R, "CT" * 4 + R)
    add("AG" * 4 + R, "CT" * 6 + R)
    add(L + "AG" * 4, L + "CT" * 6)
    add(L + "AG" * 6, L + "CT" * 4)
    add(L + "A" * 9 + R, L + "C" * 12 + R)
    add(L + "A" * 12 + R, L + "C" * 7 + R)
    add(L + "A" * 8 + R + "G" * 9 + L, L + "C" * 8 + R + "T" * 9 + L)
    add("A" * 8 + L + "G" * 8, "C" * 8 + L + "T" * 8)
    add(L + "AAAAAAAA" + "G" + R, L + "CCCCCCCC" + "T" + R)
    add("A" * 8, "C" * 8)
    add("A" * 40 + R, "C" * 3 + R)
    add("A" * 3 + R, "C" * 40 + R)
    return out


def main():
    ref_dir = os.path.join(reference_dir(), "seqan_library")
    if not os.path.isdir(ref_dir):
        sys.exit("no SeqAn at %s: this script runs only where the reference tree is present" % ref_dir)
    cs = cases()
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "driver.cpp"), os.path.join(d, "driver")
        open(src, "w").write(DRIVER)
        subprocess.check_call(["g++", "-O1", "-fpermissive", "-w", "-I" + ref_dir, "-o", exe, src])
        text = "".join("%s %s\n" % (r.hex(), h.hex()) for r, h in cs)
        lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == len(cs), (len(lines), len(cs))
    recs = []
    for (r, h), ln in zip(cs, lines):
        score, row0, row1 = ln.split(" ")
        recs.append({"ref": r.decode("latin-1"), "hap": h.decode("latin-1"), "score": int(score), "row0": row0, "row1": row1})
    with open(OUT, "w") as f:
        json.dump(recs, f, separators=(",", ":"))
    print(len(recs), "cases,", os.path.getsize(OUT), "bytes ->", OUT)


if __name__ == "__main__":
    main()
