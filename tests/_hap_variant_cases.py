"""The alignments the variants kernel (csrc/hap_variants_kernel.hip) and its host twin (host/align_haplotypes.cpp: hapVariantsHost) are
checked on, shared by tests/test_hap_variants_cpu.py and tests/test_gpu_hap_variants.py: the SeqAn fixtures, hand-written gapped rows
and seeded random mutations aligned by tests/_hapalign_oracle.py.  A case is (ref bytes, hap bytes, ref_pos list); the twin is reached
through ddh_hap_variants_json."""
import ctypes as C
import json
import os

import numpy as np

from tests import _hapalign_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 16

# hand-written alignments as gapped rows (reference, haplotype): raw letters, '-' = gap
HAND_ROWS = [
    # deletions of 1 / 2 / 3 bases in homopolymers and 2- / 3-mer repeats: the run reaches index 1, index 0, size - l
    ("CAAAAT", "C-AAAT"), ("AAAAT", "A-AAT"), ("AAAAT", "AAA-T"), ("TCAAAA", "TC-AAA"), ("TCAAAA", "TCAA-A"), ("AAAAA", "A-AAA"),
    ("GACACACT", "GAC--ACT"), ("ACACACT", "AC--ACT"), ("ACACACAC", "ACAC--AC"), ("TCAGCAGCAGG", "TCAG---CAGG"), ("CAGCAGCAG", "CAG---CAG"),
    ("CAGCAGCAG", "C---AGCAG"), ("GGACACAC", "GGAC--AC"),
    # the same as insertions
    ("CAAA-T", "CAAAAT"), ("CA-AAT", "CAAAAT"), ("A-AAA", "AAAAA"), ("AAA-A", "AAAAA"), ("GACAC--T", "GACACACT"), ("AC--ACT", "ACACACT"),
    ("ACAC--AC", "ACACACAC"), ("TCAG---CAGG", "TCAGCAGCAGG"), ("CAG---CAG", "CAGCAGCAG"), ("C---AGCAG", "CAGCAGCAG"), ("TCAAA-A", "TCAAAAA"),
    # a SNP at base 0 and at the last base; a haplotype of one base
    ("ACGT", "CCGT"), ("ACGT", "ACGA"), ("A", "C"), ("A", "A"), ("ACGT", "--G-"), ("ACGT", "T---"), ("ACGT", "---T"),
    # N, lower case and U in the reference next to a variant (flanks compare raw letters, variants seqan::Dna letters)
    ("ACnNTuAC", "AC-NTTAC"), ("acgtNNac", "acgt-Nac"), ("ACUUAC", "ACU-AC"), ("ACTUAC", "ACT-AC"), ("ACN-NAC", "ACNANAC"), ("ACu-TAC", "ACuTTAC"),
    ("ACa-AAC", "ACaAAAC"), ("ACNAC", "ACAAC"), ("ACnAC", "ACGAC"), ("AAaAT", "AA-AT"),
    # an insertion, then a deletion that starts behind it: one key, the deletion stays
    ("AC--GTAC", "ACTT--AC"), ("ACC--GTAC", "ACCTT--AC"),
    # the block substitution (deletion, then insertion) at the start, in the middle and at the end
    ("GT--ACGT", "--TTACGT"), ("ACGT--AC", "AC--TTAC"), ("ACGT--", "AC--TT"), ("ACACGT--ACAC", "ACAC--TTACAC"),
    # leading and trailing overhang
    ("--ACGT", "TTACGT"), ("ACGT--", "ACGTTT"), ("--ACGT--", "TTAC-TGG"), ("-ACGT", "GA-GT"),
    # a deletion in front of the first paired base (marked 'D', not recorded), reference bases behind the last haplotype base
    ("AACGT", "--CGT"), ("ACGTAA", "ACGT--"), ("AAC-GT", "--CTGT"),
    # an insertion as long as the reference sequence and longer: no closed form, the pair is converted on the host
    ("A---C", "ATTTC"), ("A--C", "ATTC"), ("AC----G", "ACTTTTG"),
]


def ref_pos_of_rows(row0, row1):
    pos, i = [], 0
    for a, b in zip(row0, row1):
        if b != "-":
            pos.append(i if a != "-" else -1 - i)
        if a != "-":
            i += 1
    return pos


def hand_cases():
    return [(r0.replace("-", "").encode(), r1.replace("-", "").encode(), ref_pos_of_rows(r0, r1)) for r0, r1 in HAND_ROWS]


def fixture_cases():
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "hapalign_seqan.json")))
    return [(c["ref"].encode("latin-1"), c["hap"].encode("latin-1"), ref_pos_of_rows(c["row0"], c["row1"])) for c in fx]


def random_cases(n=300, seed=20):
    """references of 1 ... 300 bases, half of them built from short repeat units, with a few SNPs, insertions and deletions"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        length = int(rng.integers(1, 301)) if k % 3 == 0 else int(rng.integers(1, 60))
        if k % 2:
            unit = "".join(rng.choice(list("ACGT"), int(rng.integers(1, 4))))
            ref = list((unit * length)[:length])
            for _ in range(int(rng.integers(0, 3))):
                ref[int(rng.integers(0, length))] = str(rng.choice(list("ACGTNacgtU")))
        else:
            ref = list(rng.choice(list("ACGT"), length))
        hap = list(ref)
        for _ in range(int(rng.integers(0, 4))):
            at = int(rng.integers(0, len(hap) + 1))
            kind = int(rng.integers(0, 3))
            if kind == 0 and at < len(hap):
                hap[at] = "ACGT"[int(rng.integers(0, 4))]
            elif kind == 1:
                l = int(rng.integers(1, 4))
                hap[at:at] = hap[at - l:at] if at >= l and rng.random() < 0.6 else list(rng.choice(list("ACGT"), l))
            elif at < len(hap) and len(hap) > 1:
                del hap[at:at + int(rng.integers(1, 4))]
        if not hap:
            hap = ["A"]
        r, h = "".join(ref).encode(), "".join(hap).encode()
        out.append((r, h, orc.align(r, h)[3]))
    return out


_cases = None


def all_cases():
    global _cases
    if _cases is None:
        _cases = fixture_cases() + hand_cases() + random_cases()
    return _cases


def twin_window(ref, haps, ref_pos, cap=CAP):
    """ddh_hap_variants_json for one window -> (summary int32 [n, 4], variants int16 [n, cap, 8], the parsed JSON)"""
    from dindel_tgi_amd import hostlib
    lib = hostlib.load()
    lib.ddh_hap_variants_json.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_char_p, C.c_int]
    flat = [p for ps in ref_pos for p in ps]
    n = len(haps)
    summary, variants = np.zeros((n, 4), np.int32), np.zeros((n, cap, 8), np.int16)
    buf = C.create_string_buffer(1 << 22)
    got = lib.ddh_hap_variants_json(ref, len(ref), b"".join(haps), (C.c_int * n)(*[len(h) for h in haps]), n, (C.c_int * max(len(flat), 1))(*flat), cap,
                                    summary.ctypes.data, variants.ctypes.data, buf, len(buf))
    assert got > 0, got
    return summary, variants, json.loads(buf.value.decode())
