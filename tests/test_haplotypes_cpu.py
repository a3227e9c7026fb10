"""Candidate haplotypes from reads without a GPU: the closed-form block table (blockTableHost) and the sequential fallback against the
literal restatement of the reference's insert-and-split process (tests/_haplotypes_oracle.py), setThresholds, generateHaplotypes, the
tool with --hostDistribution, and the C ABI of the device entry.

The restatement is not the reference: Haplotype.hpp needs Boost and HaplotypeDistribution.cpp bam.h, neither is in the image, so no
fixture can come from the reference's own code.  Parity with the reference is therefore unpinned, like the host logic of DESIGN §15."""
import ctypes as C
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

from dindel_tgi_amd import capi, hapdist, hostlib
from tests import _bamwriter, _getreads_oracle, _haplotypes_cases as cases, _haplotypes_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dindel_tgi_amd", "host", "dindel_haplotypes")
BUF = 1 << 22


@pytest.fixture(scope="module")
def host():
    lib = hostlib.load()
    B = C.POINTER(capi.dd_hap_batch)
    lib.ddh_hap_window_table_json.argtypes = [B, C.c_int, C.c_int, C.c_char_p, C.c_int]
    lib.ddh_hap_thresholds_json.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int]
    lib.ddh_hap_generate_json.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int]
    lib.ddh_hap_window_haplotypes_json.argtypes = [B, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                                   C.c_char_p, C.c_int]
    lib.ddh_haplotypes_main.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
    return lib


def _json(fn, *args):
    buf = C.create_string_buffer(BUF)
    assert fn(*args, buf, BUF) > 0
    return json.loads(buf.value.decode())


def _blocks(bl):
    return [(b[0], b[1], [(bytes.fromhex(e[0]), e[1], e[2]) for e in b[2]]) for b in bl]


def host_table(host, case, mode):
    """("ok", blocks, insertions, left), ("status", s) or ("throw", message) of the product for one window"""
    _, rs, ref, reads = case
    b = hapdist.host_batch(hapdist.pack([(rs, ref)], [reads]))
    j = _json(host.ddh_hap_window_table_json, C.byref(b), 0, mode)
    if "throw" in j:
        return ("throw", j["throw"])
    if "blocks" not in j:
        return ("status", j["status"])
    return ("ok", _blocks(j["blocks"]), _blocks(j["ins"]), j["left"])


def restated_table(case):
    o = orc.window_table(*case[1:])
    return ("ok", o[1], [(p, 0, e) for p, e in o[2]], o[3]) if o[0] == "ok" else o


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------

def test_header_additions_compile_as_c99_and_agree_with_ctypes(lib, tmp_path):
    assert lib.dd_abi_version() == 13                     # new symbols only
    bf = [n for n, _ in capi.dd_hap_batch._fields_]
    tf = [n for n, _ in capi.dd_hap_blocks._fields_]
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dindel_hmm.h"\nint main(void) {\n'
                   ' printf("%d' + " %d" * len(bf) + '\\n", (int)sizeof(dd_hap_batch)' + "".join(", (int)offsetof(dd_hap_batch, %s)" % f for f in bf) + ");\n"
                   ' printf("%d' + " %d" * len(tf) + '\\n", (int)sizeof(dd_hap_blocks)' + "".join(", (int)offsetof(dd_hap_blocks, %s)" % f for f in tf) + ");\n"
                   ' printf("%d %d %d %d %d %d %d %d\\n", DD_HAPDIST_OK, DD_HAPDIST_TOO_WIDE, DD_HAPDIST_OVERFLOW, DD_HAPDIST_HOST, DD_HAPDIST_MAX_WINDOW,\n'
                   '  DD_HAPDIST_MAX_DISTINCT, DD_HAPDIST_MAX_INS_POS, DD_HAP_BLOCKS_LOG_FIELDS);\n'
                   ' return (int)(sizeof(&dd_hap_blocks_offsets) + sizeof(&dd_hap_blocks_workspace_bytes) + sizeof(&dd_hap_blocks_device) +\n'
                   '  sizeof(&dd_hap_blocks_compute) + sizeof(&dd_hap_blocks_last_launch)) == 0; }\n')
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    l1, l2, l3 = subprocess.check_output([exe]).decode().split("\n")[:3]
    for line, S in ((l1, capi.dd_hap_batch), (l2, capi.dd_hap_blocks)):
        assert [int(x) for x in line.split()] == [C.sizeof(S)] + [getattr(S, n).offset for n, _ in S._fields_]
    assert [int(x) for x in l3.split()] == [capi.DD_HAPDIST_OK, capi.DD_HAPDIST_TOO_WIDE, capi.DD_HAPDIST_OVERFLOW, capi.DD_HAPDIST_HOST, capi.DD_HAPDIST_MAX_WINDOW,
                                            capi.DD_HAPDIST_MAX_DISTINCT, capi.DD_HAPDIST_MAX_INS_POS, len(capi.HAP_BLOCKS_LOG_FIELDS)]
    assert lib.dd_hap_blocks_workspace_bytes() == 256


GOOD = [(1000, cases.G[1000:1024]), (1100, cases.G[1100:1130])], [[(1002, 0, cases.cigar("6M2I8M"), b"ACGTACGGACGTACGT")], [(1101, 16, cases.cigar("9M"), b"ACGTACGTA")]]


def _compute(lib, a, t, break_batch=None, break_tables=None):
    b, s = hapdist.host_batch(a), hapdist.host_tables(t)
    if break_batch:
        break_batch(b)
    if break_tables:
        break_tables(s)
    return lib.dd_hap_blocks_compute(C.byref(b), C.byref(s), 0)


def test_every_validation_error_of_the_host_entry(lib):
    import torch
    good = hapdist.pack(*GOOD)
    tables = hapdist.alloc_tables(2, hapdist.offsets(good))
    INV = capi.DD_ERR_INVALID
    assert lib.dd_hap_blocks_compute(None, None, 0) == INV

    def changed(src, key, idx, val):
        a = {k: v.copy() for k, v in src.items()}
        a[key][idx] = val
        return a
    for key in ("win_ref_off", "win_read_off", "read_op_off", "read_base_off"):
        assert _compute(lib, changed(good, key, 0, 1), tables) == INV and key + " does not start at 0" in capi.last_error(), key
        assert _compute(lib, changed(good, key, 1, 10 ** 6), tables) == INV and key + " decreases" in capi.last_error(), key
    assert _compute(lib, changed(good, "win_read_off", 2, 3), tables) == INV and "does not end at n_reads" in capi.last_error()
    for f in hapdist.BATCH_FIELDS:
        assert _compute(lib, good, tables, break_batch=lambda b, f=f: setattr(b, f, None)) == INV and "null" in capi.last_error(), f
    assert _compute(lib, good, tables, break_batch=lambda b: setattr(b, "n_windows", -1)) == INV
    assert _compute(lib, good, tables, break_batch=lambda b: setattr(b, "n_reads", -1)) == INV
    for f in hapdist.WINDOW_FIELDS + hapdist.OFFSET_FIELDS + hapdist.TABLE_FIELDS:
        assert _compute(lib, good, tables, break_tables=lambda s, f=f: setattr(s, f, None)) == INV and "null" in capi.last_error(), f
    for key in hapdist.OFFSET_FIELDS:
        assert _compute(lib, good, changed(tables, key, 0, 1)) == INV and key + " does not start at 0" in capi.last_error()
        assert _compute(lib, good, changed(tables, key, 1, 10 ** 6)) == INV and key + " decreases" in capi.last_error()
    o = {k: np.zeros(3, np.int32) for k in hapdist.OFFSET_FIELDS}
    b = hapdist.host_batch(good)
    assert lib.dd_hap_blocks_offsets(C.byref(b), None, o["ent_off"].ctypes.data, o["ins_off"].ctypes.data) == INV
    assert lib.dd_hap_blocks_offsets(None, o["blk_off"].ctypes.data, o["ent_off"].ctypes.data, o["ins_off"].ctypes.data) == INV
    off = hapdist.offsets(good)
    assert off["blk_off"].tolist() == [0, 24, 54] and off["ent_off"].tolist() == [0, 160, 344] and off["ins_off"].tolist() == [0, 1, 1]
    rc = _compute(lib, good, tables)                           # a well-formed call gets as far as the device
    if not torch.cuda.is_available():
        assert rc == capi.DD_ERR_NO_DEVICE and "no HIP device" in capi.last_error()


def test_device_entry_validates_before_any_launch(lib):
    b, t = capi.dd_hap_batch(), capi.dd_hap_blocks()
    b.n_windows, b.n_reads = 1, 1
    for f in hapdist.BATCH_FIELDS:
        setattr(b, f, 4096)                                   # never dereferenced on the host
    for f, _ in capi.dd_hap_blocks._fields_:
        setattr(t, f, 4096)
    fn, INV = lib.dd_hap_blocks_device, capi.DD_ERR_INVALID
    assert fn(None, C.byref(t), 1, 1, 1, 4096, 256, None) == INV
    assert fn(C.byref(b), None, 1, 1, 1, 4096, 256, None) == INV
    assert fn(C.byref(b), C.byref(t), -1, 1, 1, 4096, 256, None) == INV and "capacity" in capi.last_error()
    assert fn(C.byref(b), C.byref(t), 1, 1, 1, None, 256, None) == INV and "workspace" in capi.last_error()
    assert fn(C.byref(b), C.byref(t), 1, 1, 1, 4096, 255, None) == INV and "workspace" in capi.last_error()
    for f in hapdist.BATCH_FIELDS:
        setattr(b, f, None)
        assert fn(C.byref(b), C.byref(t), 1, 1, 1, 4096, 256, None) == INV and "null array in the batch" in capi.last_error(), f
        setattr(b, f, 4096)
    for f, _ in capi.dd_hap_blocks._fields_:
        setattr(t, f, None)
        assert fn(C.byref(b), C.byref(t), 1, 1, 1, 4096, 256, None) == INV and "null array in the tables" in capi.last_error(), f
        setattr(t, f, 4096)
    t.entries = 4100
    assert fn(C.byref(b), C.byref(t), 1, 1, 1, 4096, 256, None) == INV and "aligned" in capi.last_error()
    b.n_windows = -1
    assert fn(C.byref(b), C.byref(t), 1, 1, 1, 4096, 256, None) == INV
    b.n_windows = 0
    assert fn(C.byref(b), C.byref(t), 1, 1, 1, None, 0, None) == capi.DD_SUCCESS
    out = (C.c_int64 * 4)()
    lib.dd_hap_blocks_last_launch(C.byref(out))              # nothing launched: readable, no device touched


# ---- the block table ----------------------------------------------------------------------------------------------------------------------

ALL_CASES = cases.hand() + cases.generated(300, 1) + cases.generated(20, 2, wide=True)


def test_the_cases_hold_what_they_must():
    """the generator and the hand cases cover the list the comparison is meant for"""
    names = {c[0] for c in cases.hand()}
    for need in ("zero_reads", "on_grid", "off_grid", "past_both_ends", "ref_read_and_snp", "n_in_read", "leading_clip_overlaps_its_match",
                 "trailing_clip_runs_on", "hard_clips", "del_1_29_30_31", "ref_skip", "ins_first_read_creates", "ins_middle_read_creates",
                 "ins_last_read_creates", "ins_carrier_goes_on_behind_its_match", "two_insertions_at_one_position", "mate_unmapped_is_ignored",
                 "no_operations", "pad_throws"):
        assert need in names, need
    ops = [op for c in ALL_CASES for rd in c[3] for op in rd[2]]
    for op in range(7):
        assert any(o == op for o, _ in ops), op
    assert {1, 29, 30, 31} <= {n for o, n in ops if o == 2}
    assert any(rd[1] & 8 for c in ALL_CASES for rd in c[3]) and any(not rd[2] for c in ALL_CASES for rd in c[3])
    assert any(rd[0] < c[1] for c in ALL_CASES for rd in c[3]) and any(b"N" in rd[3] for c in ALL_CASES for rd in c[3])
    assert len(ALL_CASES) > 300


def test_closed_form_and_sequential_path_equal_the_restatement_on_every_window(host):
    seen = {"ok": 0, "throw": 0, "status": 0, "ins": 0, "left": set()}
    for case in ALL_CASES:
        want = restated_table(case)
        closed, seq = host_table(host, case, 0), host_table(host, case, 1)
        assert seq == want, case[0]
        if want[0] == "throw":
            assert closed == ("status", capi.DD_HAPDIST_HOST), case[0]
            seen["throw"] += 1
        elif closed[0] == "status":                            # too many strings in a block, too many insertion positions: the fallback's
            assert closed[1] == capi.DD_HAPDIST_OVERFLOW, case[0]
            seen["status"] += 1
        else:
            assert closed == want, case[0]
            seen["ok"] += 1
            seen["ins"] += len(want[2])
            seen["left"].add(want[3])
    assert seen["ok"] > 280 and seen["throw"] >= 5 and seen["ins"] > 100 and seen["left"] == {0, 2, 3}, seen


def test_hand_cases_by_their_numbers(host):
    by = {c[0]: c for c in cases.hand()}
    t = host_table(host, by["zero_reads"], 0)
    assert t[0] == "ok" and [(b[0], b[1]) for b in t[1]] == [(4 * k, 4) for k in range(6)] and all(b[2] == [(cases.G[1000 + b[0]:1004 + b[0]], 1, True)] for b in t[1])
    assert t[2] == [] and t[3] == 0
    t = host_table(host, by["leading_clip_overlaps_its_match"], 0)       # 5S12M at 1004: positions 1004 ... 1008 are shown twice
    counts = {b[0]: sum(e[1] for e in b[2]) for b in t[1]}
    assert counts[4] == 3 and counts[8] == 3 and counts[9] == 2 and counts[12] == 2 and counts[16] == 1 and 9 in counts
    t = host_table(host, by["del_1_29_30_31"], 0)
    at = {b[0]: {e[0]: e[1] for e in b[2]} for b in t[1] if b[1] == 1}
    assert at[8][b"$"] == 1 and at[10][b"@"] == 1 and at[10][b"A"] >= 1 and at[11][b"A"] >= 2        # '#' + 1, 29, 30, and 31 / 45 cut to 30
    assert 1011 + 30 - 1000 in {b[0] for b in t[1]} and 1011 + 31 - 1000 not in {b[0] for b in t[1]}  # ... which advance by 30 only: 5M45D5M goes on at 1041
    assert host_table(host, by["pad_throws"], 1) == ("throw", "I don't know how to smoke this CIGAR")
    assert host_table(host, by["mag_niet"], 1) == ("throw", "Mag niet.")
    assert host_table(host, by["left_gap_before_window"], 0)[3] == 2 and host_table(host, by["left_touching"], 0)[3] == 3
    # the first carrier creates the position: crossings are counted from then on only
    first, last = host_table(host, by["ins_first_read_creates"], 0)[2], host_table(host, by["ins_last_read_creates"], 0)[2]
    assert first == [(8, 0, [(b"", 3, True), (b"GG", 1, False)])] and last == [(8, 0, [(b"", 1, True), (b"GG", 1, False)])]
    assert host_table(host, by["ins_middle_read_creates"], 0)[2] == [(8, 0, [(b"", 2, True), (b"GG", 2, False)])]
    assert host_table(host, by["ins_carrier_goes_on_behind_its_match"], 0)[2] == [(8, 0, [(b"", 3, True), (b"TT", 2, False)])]
    two = host_table(host, by["two_insertions_at_one_position"], 0)[2]
    assert two == [(8, 0, [(b"", 2, True), (b"ACA", 1, False), (b"GG", 2, False)])]


def test_widths_and_caps_give_the_statuses(host):
    wide = ("wide", 1000, cases.G[1000:1000 + capi.DD_HAPDIST_MAX_WINDOW + 1], [(1010, 0, cases.cigar("20M"), cases.G[1010:1030])])
    assert host_table(host, wide, 0) == ("status", capi.DD_HAPDIST_TOO_WIDE)
    assert host_table(host, wide, 1) == restated_table(wide)
    ref = cases.G[2000:2016]
    others = [bytes(b"ACGT"[(x >> s) & 3] for s in (6, 4, 2, 0)) for x in range(40)]
    others = [s for s in others if s != ref[4:8]]
    for n, status in ((capi.DD_HAPDIST_MAX_DISTINCT - 1, None), (capi.DD_HAPDIST_MAX_DISTINCT, capi.DD_HAPDIST_OVERFLOW)):
        case = ("d", 2000, ref, [(2004, 0, [(0, 4)], s) for s in others[:n]])
        got = host_table(host, case, 0)
        assert (got == ("status", status)) if status else (got == restated_table(case) and len(got[1][1][2]) == capi.DD_HAPDIST_MAX_DISTINCT)
        assert host_table(host, case, 1) == restated_table(case)
    many = ("i", 1000, cases.G[1000:1100], [(1000 + k, 0, cases.cigar("1M1I1M"), b"ACG") for k in range(capi.DD_HAPDIST_MAX_INS_POS + 1)])
    assert host_table(host, many, 0) == ("status", capi.DD_HAPDIST_OVERFLOW) and host_table(host, many, 1) == restated_table(many)
    assert host_table(host, ("i", 1000, cases.G[1000:1100], many[3][:-1]), 0) == restated_table(("i", 1000, cases.G[1000:1100], many[3][:-1]))


# ---- setThresholds and generateHaplotypes ------------------------------------------------------------------------------------------------------

def blocks_text(blocks):
    """blocks: [(start, end, insertion, [(seq, count, is_ref)])] -> the hook's text, with the frequencies setFrequencies gives"""
    out = []
    for start, end, ins, ent in blocks:
        out.append("B %d %d %d" % (start, end, int(ins)))
        total = sum(e[1] for e in ent)
        out += ["E %s %d %d %r" % (e[0].hex() or "-", e[1], int(e[2]), float(e[1]) / float(total)) for e in ent]
    return "\n".join(out).encode()


def restated_iterator(blocks):
    it = orc.Iterator2.__new__(orc.Iterator2)
    it.hbs = []
    for start, end, ins, ent in blocks:
        e = orc._HB()
        e.start, e.end, e.type = start, end, orc.BLOCK_INSERT if ins else orc.BLOCK_NORMAL
        total = sum(x[1] for x in ent)
        for seq, cnt, is_ref in ent:
            h = orc.Hap(orc.REF if is_ref else orc.NORMAL, seq)
            h.freq = float(cnt) / float(total)
            e.haps.append(h)
        it.hbs.append(e)
    return it


THRESHOLD_TABLES = {
    "ties": [(100, 103, False, [(b"ACGT", 6, True), (b"ACTT", 2, False), (b"AGGT", 2, False)]), (104, 105, False, [(b"AA", 8, False), (b"AC", 2, True)]),
             (106, 106, False, [(b"$", 2, False), (b"G", 6, True), (b"T", 2, False)])],
    "single_entries": [(100, 103, False, [(b"ACGT", 5, True)]), (104, 107, False, [(b"AAAA", 1, True)]), (108, 109, False, [(b"CC", 3, True), (b"CG", 3, False)])],
    "insertion": [(100, 103, False, [(b"ACGT", 9, True), (b"ACGA", 1, False)]), (104, 103, True, [(b"", 7, True), (b"GG", 2, False), (b"GT", 1, False)]),
                  (104, 107, False, [(b"CCCC", 4, True), (b"CCCA", 3, False), (b"CCCG", 3, False)])],
    "no_reference": [(100, 101, False, [(b"AC", 1, False), (b"AG", 3, False)])],
}


@pytest.mark.parametrize("name", sorted(THRESHOLD_TABLES))
@pytest.mark.parametrize("max_hap", [1, 2, 8])
def test_set_thresholds_equals_the_restatement(host, name, max_hap):
    blocks = THRESHOLD_TABLES[name]
    it = restated_iterator(blocks)
    got = _json(host.ddh_hap_thresholds_json, blocks_text(blocks), max_hap)
    try:
        it.set_thresholds(max_hap)
    except orc.Thrown as e:
        assert got == {"throw": str(e)} and name == "no_reference"
        return
    assert got["logNumHap"] == it.log_num_hap
    assert [[bytes.fromhex(e[0]) for e in b[2]] for b in got["blocks"]] == [[h.seq for h in e.haps] for e in it.hbs]
    if name == "ties" and max_hap == 2:                        # the first minimum, the first string at or below it in map order, one at a time
        assert [[bytes.fromhex(e[0]) for e in b[2]] for b in got["blocks"]] == [[b"ACGT"], [b"AA", b"AC"], [b"G"]]


GEN_BLOCKS = [(100, 103, False, [(b"ACGT", 6, True), (b"ACTT", 2, False)]), (104, 103, True, [(b"", 7, True), (b"GG", 2, False)]),
              (104, 104, False, [(b"%", 2, False), (b"C", 6, True)]), (105, 108, False, [(b"TTAG", 8, True)]), (109, 111, False, [(b"CAT", 5, True), (b"CGT", 1, False)])]
GEN_VARIANTS = {
    "del": [(106, "-TA", 0)], "ins": [(102, "+AAC", 0)], "snp": [(110, "A=>G", 0), (101, "C=>C", 0)],
    "comb_on": [(106, "-TA", 1), (102, "+AAC", 1), (110, "A=>T", 1)], "comb_mixed": [(106, "-TA", 0), (102, "+AAC", 1), (110, "A=>T", 0)],
    "position_deleted": [(105, "+G", 0), (106, "T=>A", 1)],         # the '%' deletion takes 104 and 105 away in some combinations
    "nowhere": [(300, "-A", 0)], "none": [],
}


@pytest.mark.parametrize("name", sorted(GEN_VARIANTS))
@pytest.mark.parametrize("to_n", [False, True])
def test_generate_haplotypes_equals_the_restatement(host, name, to_n):
    it = restated_iterator(GEN_BLOCKS)
    it.max = [len(e.haps) for e in it.hbs]
    variants = GEN_VARIANTS[name]
    want = it.generate([(p, "DEL" if s[0] == "-" else "INS" if s[0] == "+" else "SNP", s[1:].encode() if s[0] in "+-" else s.encode(), c) for p, s, c in variants], to_n)
    got = _json(host.ddh_hap_generate_json, blocks_text(GEN_BLOCKS), "\n".join("%d %s %d" % v for v in variants).encode(), int(to_n))
    assert [bytes.fromhex(h) for h in got["haps"]] == want and len(want) >= 8
    assert b"ACGTCTTAGCAT" in want and want == sorted(want)
    if name == "ins":
        assert (b"ACNNNGTCTTAGCAT" in want) == to_n and (b"ACAACGTCTTAGCAT" in want) != to_n
    if name == "none":
        assert b"ACGTTAGCAT" in want                           # '%' = '#' + 2: itself and the base behind it


def _variants_for(rng, rs, L):
    out = []
    for _ in range(rng.randrange(1, 4)):
        p = rs + rng.randrange(0, L)
        kind = rng.randrange(3)
        out.append((p, "-" + "A" * rng.randrange(1, 4) if kind == 0 else "+" + "".join(rng.choice("ACGT") for _ in range(rng.randrange(1, 4))) if kind == 1
                    else "%s=>%s" % (chr(cases.G[p]), rng.choice("ACGT")), rng.randrange(2)))
    return out


def test_windows_end_to_end_equal_the_restatement(host):
    """selectBlocks, setThresholds, the two skip tests and generateHaplotypes behind both table paths, on the generated windows"""
    rng = random.Random(77)
    seen = {"ok": 0, "skip": 0, "throw": 0}
    for case in cases.hand() + cases.generated(120, 3, max_reads=25):
        _, rs, ref, reads = case
        L = len(ref)
        left = rs + rng.choice([0, 0, min(3, L - 1), min(20, L - 1)])
        right = max(left, rs + L - 1 - rng.choice([0, 0, 2, 20]))
        variants = _variants_for(rng, rs, L)
        max_hap, skip_max, prod = rng.choice([1, 2, 8, 8]), rng.choice([200, 200, 4]), rng.choice([1e7, 1e7, 40.0])
        want = orc.get_haplotypes(rs, ref, reads, (left + right) // 2, left, right,
                                  [(p, "DEL" if s[0] == "-" else "INS" if s[0] == "+" else "SNP", s[1:].encode() if s[0] in "+-" else s.encode(), c) for p, s, c in variants],
                                  max_hap, skip_max, prod, False)
        if want == ("throw", "undefined: hapBlocks[-1]"):      # unpinned: the reference reads in front of its vector
            continue
        b = hapdist.host_batch(hapdist.pack([(rs, ref)], [reads]))
        text = "\n".join("%d %s %d" % v for v in variants).encode()
        for mode in (0, 1):
            got = _json(host.ddh_hap_window_haplotypes_json, C.byref(b), 0, mode, left, right, text, len(reads), max_hap, skip_max, prod, 0)
            if want[0] == "ok":
                assert (got.get("left"), got.get("right"), [bytes.fromhex(h) for h in got.get("haps", [])]) == want[1:], (case[0], mode, got)
            elif want[0] == "skip":
                assert got.get("message", "").startswith(want[1]), (case[0], mode, got, want)
            else:
                assert got == {"message": want[1]}, (case[0], mode, got, want)
        seen[want[0]] += 1
    assert seen["ok"] > 60 and seen["skip"] >= 5 and seen["throw"] >= 3, seen


# ---- the tool -----------------------------------------------------------------------------------------------------------------------------

def run_tool(args):
    env = dict(os.environ)
    try:
        import torch
        env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    except ImportError:
        pass
    p = subprocess.run([TOOL] + [str(a) for a in args], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def parse_wrh(text):
    wins = []
    for line in text.split("\n"):
        if line.startswith("W "):
            _, idx, left, right = line.split()
            wins.append({"index": int(idx), "left": int(left), "right": int(right), "ref": None, "haps": []})
        elif line.startswith("R "):
            wins[-1]["ref"] = line[2:]
        elif line.startswith("H "):
            wins[-1]["haps"].append(line[2:])
        else:
            assert line == "", line
    return wins


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    """One target, single-end reads with mapping qualities that differ inside every window (the order of getReads is then pinned), a
    deletion, an insertion and a SNP carried by some of them."""
    tmp = tmp_path_factory.mktemp("haps")
    rng = random.Random(4)
    target = "".join(rng.choice("ACGT") for _ in range(6000))
    fasta = str(tmp / "t.fa")
    with open(fasta, "w") as f:
        f.write(">chrT\n" + "\n".join(target[i:i + 60] for i in range(0, len(target), 60)) + "\n")
    with open(fasta + ".fai", "w") as f:
        f.write("chrT\t%d\t6\t60\t61\n" % len(target))
    records = []
    for k, pos in enumerate(sorted(rng.randrange(2600, 4700) for _ in range(150))):
        seq, cig = target[pos:pos + 60], "60M"
        if pos <= 3080 and pos + 60 > 3120 and k % 2:
            at = 3100 - pos
            seq, cig = target[pos:3100] + target[3103:pos + 63], "%dM3D%dM" % (at, 60 - at)
        elif pos <= 3380 and pos + 60 > 3420 and k % 2:
            at = 3400 - pos
            seq, cig = target[pos:3400] + "GA" + target[3400:pos + 58], "%dM2I%dM" % (at, 58 - at)
        elif pos <= 3700 < pos + 60 and k % 2:
            seq = seq[:3700 - pos] + ("A" if target[3700] != "A" else "C") + seq[3701 - pos:]
        if k % 13 == 5:
            seq, cig = "TTT" + seq, "3S" + cig
        records.append((0, dict(qname="r%d" % k, flag=16 if k % 3 == 0 else 0, pos=pos, mapq=21 + (k * 7) % 39, cigar=cig, seq=seq, qual=[30] * len(seq),
                                mtid=-1, mpos=-1, isize=0, tags={})))
    bam = str(tmp / "s.bam")
    _bamwriter.write_bam(bam, "@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:chrT\tLN:%d\n" % len(target), [("chrT", len(target))], records)
    windows = [(3040, 3160, [(3100, "-" + target[3100:3103])]), (3340, 3460, [(3400, "+GA")]), (3640, 3760, [(3700, "%s=>%s" % (target[3700], "A" if target[3700] != "A" else "C"))]),
               (5440, 5560, [(5500, "-A")])]
    var = str(tmp / "w.txt")
    with open(var, "w") as f:
        for left, right, vs in windows:
            f.write("chrT %d %d %s\n" % (left, right, " ".join("%d,%s" % v for v in vs)))
    return dict(tmp=tmp, target=target, fasta=fasta, bam=bam, var=var, windows=windows, records=[r for _, r in records])


def test_tool_with_host_distribution_equals_the_restatement(sample, host):
    out = str(sample["tmp"] / "haps.txt")
    args = ["--bamFile", sample["bam"], "--ref", sample["fasta"], "--varFile", sample["var"], "--outputFile", out, "--hostDistribution", "--quiet", "--batchWindows", "2"]
    argv = (C.c_char_p * (len(args) + 2))(b"dindel_haplotypes", *[a.encode() for a in args], None)
    assert host.ddh_haplotypes_main(len(args) + 1, argv) == 0
    got = parse_wrh(open(out).read())
    by_name = {r["qname"]: r for r in sample["records"]}
    picked = _getreads_oracle.run_windows(sample["records"], [(w[0], w[1]) for w in sample["windows"]])
    want = []
    for k, ((left, right, vs), sel) in enumerate(zip(sample["windows"], picked)):
        if isinstance(sel, dict):
            continue                                           # the last window: too few reads
        mq = [x[2] for x in sel]
        assert len(set(mq)) == len(mq)                         # no ties: the order is the reference's
        reads = [(by_name[x[0]]["pos"], by_name[x[0]]["flag"], [(op, ln) for ln, op in _bamwriter.parse_cigar(by_name[x[0]]["cigar"])], by_name[x[0]]["seq"].encode()) for x in sel]
        rs, re_ = max(left - 20, 0), right + 20
        res = orc.get_haplotypes(rs, sample["target"][rs:re_ + 1].encode(), reads, left + (right - left) // 2, left, right,
                                 [(p, "DEL" if s[0] == "-" else "INS" if s[0] == "+" else "SNP", s[1:].encode() if s[0] in "+-" else s.encode(), 0) for p, s in vs])
        assert res[0] == "ok", res
        want.append({"index": k + 1, "left": res[1], "right": res[2], "ref": sample["target"][res[1]:res[2] + 1], "haps": [h.decode() for h in res[3]]})
    assert got == want and len(got) == 3
    t = sample["target"]
    for w, planted in zip(got, (t[w["left"]:3100] + t[3103:w["right"] + 1] for w in got[:1])):
        assert w["ref"] in w["haps"] and planted in w["haps"]
    assert got[1]["ref"][:3400 - got[1]["left"]] + "GA" + got[1]["ref"][3400 - got[1]["left"]:] in got[1]["haps"]
    # the binary writes the same bytes, and names the window it skips
    out2 = str(sample["tmp"] / "haps2.txt")
    rc, _, err = run_tool(["--bamFile", sample["bam"], "--ref", sample["fasta"], "--varFile", sample["var"], "--outputFile", out2, "--hostDistribution"])
    assert rc == 0 and open(out2).read() == open(out).read() and "too_few_reads" in err and "3 written" in err


def test_tool_help_and_option_errors(tmp_path):
    rc, out, _ = run_tool(["--help"])
    assert rc == 0
    for opt in ("--bamFile", "--bamFiles", "--ref", "--varFile", "--varFileIsOneBased", "--maxRead", "--maxReadLength", "--minReadOverlap", "--mapQualThreshold",
                "--filterReadAux", "--libFile", "--outputFile", "--maxHap", "--skipMaxHap", "--maxHapReadProd", "--changeINStoN", "--batchWindows", "--device",
                "--hostDistribution", "--quiet", "--help"):
        assert opt in out, opt
    o = str(tmp_path / "o")
    for args, code, text in (
            (["--ref", "r.fa", "--varFile", "v", "--outputFile", o], 1, "Error: Specify either --bamFile or --bamFiles."),
            (["--bamFile", "x.bam", "--varFile", "v", "--outputFile", o], 1, "Please specify --ref"),
            (["--bamFile", "x.bam", "--ref", "r.fa", "--outputFile", o], 1, "Please specify --varFile"),
            (["--bamFile", "x.bam", "--ref", "r.fa", "--varFile", "v"], 1, "Please specify --outputFile"),
            (["--bamFile", "x.bam", "--ref", "r.fa", "--varFile", "v", "--outputFile", o, "--batchWindows", "0"], 2, "--batchWindows"),
            (["--bamFile", "x.bam", "--ref", "r.fa", "--varFile", "v", "--outputFile", o, "--maxHap", "0"], 2, "--maxHap"),
            (["--bamFile", "x.bam", "--ref", "r.fa", "--varFile", "v", "--outputFile", o, "--skipMaxHap", "0"], 2, "--skipMaxHap"),
            (["--frobnicate"], 2, "unknown or incomplete option --frobnicate"),
            (["--bamFile"], 2, "unknown or incomplete option --bamFile"),
            (["--bamFile", str(tmp_path / "none.bam"), "--ref", "r.fa", "--varFile", "v", "--outputFile", o], 1, "Cannot open BAM file."),
            (["--bamFiles", str(tmp_path / "none.txt"), "--ref", "r.fa", "--varFile", "v", "--outputFile", o], 1, "File open error.")):
        rc, out, err = run_tool(args)
        assert rc == code and text in err, (args, rc, err)


def test_citations_of_the_new_files_point_inside_the_reference():
    nlines = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_line_counts.json")))["nlines"]
    pat = re.compile(r"((?:python/)?[A-Za-z][A-Za-z0-9_]*\.(?:cpp|hpp|py|h))`?:(\d+)(?:-(\d+))?")
    n = 0
    for rel in ("dindel_tgi_amd/csrc/hapdist_kernel.hip", "dindel_tgi_amd/csrc/hapdist_kernel.h", "dindel_tgi_amd/csrc/hapdist_host.cpp",
                "dindel_tgi_amd/host/haplotypes.hpp", "dindel_tgi_amd/host/haplotypes.cpp", "dindel_tgi_amd/host/haplotypes_main.cpp",
                "dindel_tgi_amd/host/haplotypes_capi.cpp", "dindel_tgi_amd/host/dindel_haplotypes.cpp", "tests/_haplotypes_oracle.py"):
        for m in pat.finditer(open(os.path.join(ROOT, rel)).read()):
            name, a, b = m.group(1), int(m.group(2)), int(m.group(3) or m.group(2))
            if name in nlines:
                n += 1
                assert 1 <= a <= b <= nlines[name], (rel, m.group(0), nlines[name])
    assert n >= 12, n
