"""CPU-side checks of the haplotype alignment feature: the header additions, the validation of dd_align_* (no launch is reached), the
checker itself against the output of the reference's SeqAn library (tests/golden/hapalign_seqan.json), the host conversion
(host/align_haplotypes.cpp through ddh_align_haplotypes_json) against the Python restatement and against hand-derived expectations,
the R record of the shared parser, the tool's command line, and the W / R / H dump block of INTEGRATION section 8."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from dindel_tgi_amd import capi, hapalign, hostlib
from tests import _hapalign_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dindel_tgi_amd", "host")
FIXTURES = json.load(open(os.path.join(ROOT, "tests", "golden", "hapalign_seqan.json")))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------

def test_header_compiles_as_c99_and_layout_agrees_with_ctypes(lib, tmp_path):
    assert lib.dd_abi_version() == 13                     # new symbols only: the ABI number does not move
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dindel_hmm.h"\n'
                   'int main(void) { dd_align_batch b; dd_align_result r; (void)b; (void)r;\n'
                   ' printf("%d %d %d %d %d %d %d %d %d %d\\n", (int)sizeof(dd_align_batch), (int)offsetof(dd_align_batch, ref_off),\n'
                   '  (int)offsetof(dd_align_batch, ref_seq), (int)offsetof(dd_align_batch, n_pairs), (int)offsetof(dd_align_batch, pair_ref),\n'
                   '  (int)offsetof(dd_align_batch, hap_off), (int)offsetof(dd_align_batch, hap_seq), (int)sizeof(dd_align_result),\n'
                   '  (int)offsetof(dd_align_result, status), (int)offsetof(dd_align_result, ref_pos));\n'
                   ' printf("%d %d %d %d %d\\n", DD_ALIGN_OK, DD_ALIGN_EMPTY, DD_ALIGN_TOO_LONG, DD_ALIGN_BAD_REF, DD_ALIGN_LOG_FIELDS);\n'
                   ' return 0; }\n')
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    l1, l2 = subprocess.check_output([exe]).decode().split("\n")[:2]
    B, R = capi.dd_align_batch, capi.dd_align_result
    assert [int(x) for x in l1.split()] == [C.sizeof(B), B.ref_off.offset, B.ref_seq.offset, B.n_pairs.offset, B.pair_ref.offset, B.hap_off.offset,
                                            B.hap_seq.offset, C.sizeof(R), R.status.offset, R.ref_pos.offset]
    assert [int(x) for x in l2.split()] == [capi.DD_ALIGN_OK, capi.DD_ALIGN_EMPTY, capi.DD_ALIGN_TOO_LONG, capi.DD_ALIGN_BAD_REF,
                                            len(capi.ALIGN_LOG_FIELDS)]


def _call(lib, a, result=True, break_=None):
    b = hapalign.host_batch(a)
    if break_:
        break_(b)
    n, nb = b.n_pairs, int(a["hap_off"][-1])
    out = {"score": np.zeros(max(n, 1), np.int32), "status": np.zeros(max(n, 1), np.int32), "ref_pos": np.zeros(max(nb, 1), np.int16)}
    r = capi.dd_align_result(out["score"].ctypes.data, out["status"].ctypes.data, out["ref_pos"].ctypes.data)
    if result is not True:
        result(r)
    return lib.dd_align_haplotypes(C.byref(b), C.byref(r), 0), lib.dd_align_workspace_bytes(C.byref(b))


def test_every_validation_error_is_returned(lib):
    import torch
    good = hapalign.pack([b"ACGTACGT", b"TTGCA"], [b"ACGTCGT", b"TTGGCA", b"ACGT"], [0, 1, 0])
    INV = capi.DD_ERR_INVALID
    assert lib.dd_align_haplotypes(None, None, 0) == INV and lib.dd_align_workspace_bytes(None) == 0

    def changed(key, idx, val):
        a = {k: v.copy() for k, v in good.items()}
        a[key][idx] = val
        return a
    for a, what in ((changed("ref_off", 0, 1), "ref_off does not start at 0"), (changed("hap_off", 0, 2), "hap_off does not start at 0"),
                    (changed("ref_off", 1, 20), "ref_off decreases"), (changed("hap_off", 2, 3), "hap_off decreases"),
                    (changed("pair_ref", 1, 2), "pair_ref out of range"), (changed("pair_ref", 2, -1), "pair_ref out of range")):
        rc, ws = _call(lib, a)
        assert rc == INV and ws == 0 and what in capi.last_error(), (what, capi.last_error())
    for field in ("ref_off", "ref_seq", "pair_ref", "hap_off", "hap_seq"):
        rc, ws = _call(lib, good, break_=lambda b, f=field: setattr(b, f, None))
        assert rc == INV and ws == 0 and "null" in capi.last_error(), field
    rc, _ = _call(lib, good, break_=lambda b: setattr(b, "n_pairs", -1))
    assert rc == INV
    for field in ("score", "status", "ref_pos"):
        rc, ws = _call(lib, good, result=lambda r, f=field: setattr(r, f, None))
        assert rc == INV and ws > 0 and "null" in capi.last_error(), field
    b = hapalign.host_batch(good)
    assert lib.dd_align_haplotypes(C.byref(b), None, 0) == INV
    # the well-formed batch gets as far as the device
    rc, ws = _call(lib, good)
    # one workgroup of four tiles of (8 + 64) x 7 bytes, rounded up to 256, behind the header
    assert ws == 256 + 4 * 512
    if not torch.cuda.is_available():
        assert rc == capi.DD_ERR_NO_DEVICE and "no CPU fallback" in capi.last_error()


def test_workspace_rule(lib):
    """tile = (longest reference + 64) x (longest haplotype) rounded up to 256; 4 wavefronts per workgroup, one wavefront per pair up to
    2,048 workgroups, fewer while the tiles exceed 512 MiB, never fewer than one workgroup; over-long sequences do not count"""
    def ws(ref_lens, hap_lens):
        a = {"ref_off": np.concatenate([[0], np.cumsum(ref_lens)]).astype(np.int32), "hap_off": np.concatenate([[0], np.cumsum(hap_lens)]).astype(np.int32),
             "pair_ref": np.zeros(len(hap_lens), np.int32), "ref_seq": np.zeros(1, np.uint8), "hap_seq": np.zeros(1, np.uint8)}
        return lib.dd_align_workspace_bytes(C.byref(hapalign.host_batch(a)))

    def tile(r, h):
        return ((r + 64) * h + 255) // 256 * 256
    assert ws([125], [130] * 8) == 256 + 8 * tile(125, 130)
    assert ws([125], [130] * 9) == 256 + 12 * tile(125, 130)
    assert ws([125], [130] * 100000) == 256 + 2048 * 4 * tile(125, 130)
    big = tile(4094, 4094)
    fit = (512 << 20) // (4 * big)
    assert fit == 7 and ws([4094], [4094] * 1000) == 256 + fit * 4 * big
    assert ws([4094], [4094]) == 256 + 4 * big
    assert ws([5000, 100], [50, 4095]) == 256 + 4 * tile(100, 50)


def test_device_entry_validates_before_any_launch(lib):
    b, r = capi.dd_align_batch(), capi.dd_align_result()
    b.n_refs, b.n_pairs = 1, 1
    for f in ("ref_off", "ref_seq", "pair_ref", "hap_off", "hap_seq"):
        setattr(b, f, 4096)                                   # never dereferenced on the host
    for f in ("score", "status", "ref_pos"):
        setattr(r, f, 4096)
    fn, INV = lib.dd_align_haplotypes_device, capi.DD_ERR_INVALID
    assert fn(None, C.byref(r), 10, 10, 4096, 1 << 20, None) == INV
    assert fn(C.byref(b), C.byref(r), 0, 10, 4096, 1 << 20, None) == INV
    assert fn(C.byref(b), C.byref(r), 10, capi.DD_LONG_MAX_HAP_LEN + 1, 4096, 1 << 20, None) == INV
    assert fn(C.byref(b), C.byref(r), 10, 10, None, 1 << 20, None) == INV and "workspace" in capi.last_error()
    need = 256 + 4 * 768                                      # (10 + 64) x 10 = 740 -> 768 per tile
    assert fn(C.byref(b), C.byref(r), 10, 10, 4096, need - 1, None) == INV and "too small" in capi.last_error()
    r.status = None
    assert fn(C.byref(b), C.byref(r), 10, 10, 4096, need, None) == INV and "null array" in capi.last_error()


# ---- the checker against the reference's library -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def oracle_alignments():
    """the restatement's answer for every fixture, computed once"""
    return [orc.align(c["ref"].encode("latin-1"), c["hap"].encode("latin-1")) for c in FIXTURES]


def test_fixture_file_holds_the_case_list():
    assert 300 <= len(FIXTURES) <= 400 and os.path.getsize(os.path.join(ROOT, "tests", "golden", "hapalign_seqan.json")) < 200 * 1024
    lens = [len(c[k]) for c in FIXTURES for k in ("ref", "hap")]
    assert min(lens) == 1 and 250 <= max(lens) <= 300
    # the two placements the tie rules decide, as recorded from the library: a deletion in a repeat goes to the front, an insertion into a
    # homopolymer to the end
    by = {(c["ref"], c["hap"]): c for c in FIXTURES}
    assert by[("ACACACACGT", "ACACACGT")]["row1"] == "--ACACACGT" and by[("A" * 8, "A" * 10)]["row0"] == "A" * 8 + "--"
    assert by[("A" * 10, "A" * 9)]["score"] == -969          # nine matches and a one-base gap
    for c in FIXTURES:                                        # well-formed: rows of one length, no column of two gaps, the sequences' letters
        assert len(c["row0"]) == len(c["row1"]) and all(a != "-" or b != "-" for a, b in zip(c["row0"], c["row1"]))
        assert c["row0"].replace("-", "") == orc.dna(c["ref"].encode("latin-1")) and c["row1"].replace("-", "") == orc.dna(c["hap"].encode("latin-1"))


def test_oracle_reproduces_every_seqan_fixture(oracle_alignments):
    for c, (score, row0, row1, pos) in zip(FIXTURES, oracle_alignments):
        assert (score, row0, row1) == (c["score"], c["row0"], c["row1"]), c
        ref, hap = c["ref"].encode("latin-1"), c["hap"].encode("latin-1")
        assert orc.rows_from_ref_pos(ref, hap, pos) == (row0, row1) and hapalign.gapped_rows(ref, hap, pos) == (row0, row1), c


# ---- the host conversion -------------------------------------------------------------------------------------------------------------------

def ref_pos_of_rows(row0, row1):
    pos, i = [], 0
    for a, b in zip(row0, row1):
        if b != "-":
            pos.append(i if a != "-" else -1 - i)               # a gap-facing base records the reference bases left of it
        if a != "-":
            i += 1
    return pos


def host_window(ref, haps, ref_pos):
    """ddh_align_haplotypes_json for one window; ref, haps: bytes; ref_pos: per haplotype the list of offsets"""
    lib = hostlib.load()
    lib.ddh_align_haplotypes_json.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_int, C.c_char_p, C.c_int]
    flat = [p for ps in ref_pos for p in ps]
    buf = C.create_string_buffer(1 << 22)
    n = lib.ddh_align_haplotypes_json(ref, len(ref), b"".join(haps), (C.c_int * len(haps))(*[len(h) for h in haps]), len(haps),
                                      (C.c_int * max(len(flat), 1))(*flat), 0, buf, len(buf))
    assert n > 0, n
    return json.loads(buf.value.decode())


def oracle_window(ref, haps):
    kept = orc.window(ref.decode("latin-1"), [h.decode("latin-1") for h in haps])
    return {"kept": [{"index": ml.index, "align": ml.align, "refHpos": ml.hpos,
                      "indels": [[k, ml.indels[k].str] + ml.indels[k].coords for k in sorted(ml.indels)],
                      "snps": [[k, ml.snps[k].str] + ml.snps[k].coords for k in sorted(ml.snps)]} for _, ml in kept]}


def test_host_conversion_equals_restatement_on_all_fixtures():
    """every fixture as a window of its own, then the fixtures that share a reference as one window each (variants collected across
    haplotypes, dropped ones included; *REF / R=>x entries; duplicate-reference removal)"""
    groups = {}
    for c in FIXTURES:
        ref, hap = c["ref"].encode("latin-1"), c["hap"].encode("latin-1")
        pos = ref_pos_of_rows(c["row0"], c["row1"])
        assert host_window(ref, [hap], [pos]) == oracle_window(ref, [hap]), c
        groups.setdefault(ref, []).append((hap, pos))
    shared = {r: g for r, g in groups.items() if len(g) > 1}
    assert len(shared) >= 8 and max(len(g) for g in shared.values()) >= 10
    n_dropped = n_dup = 0
    for ref, g in shared.items():
        g = g + [(ref, list(range(len(ref))))] * 2                         # and the reference itself, twice
        got = host_window(ref, [h for h, _ in g], [p for _, p in g])
        want = oracle_window(ref, [h for h, _ in g])
        assert got == want, ref
        kept = [k["index"] for k in got["kept"]]
        n_dropped += len(g) - len(kept)
        n_dup += (len(g) - 1) not in kept
        assert all(len(k["indels"]) == len(k["snps"]) == len(got["kept"][0]["indels"]) for k in got["kept"])      # every position on every kept haplotype
    assert n_dropped > 10 and n_dup == len(shared)


REF10 = b"ACGTCATGCA"


def test_hand_derived_conversions():
    """worked by hand from ObservationModelSeqAn.hpp:142-269, :37-139 and Haplotype.hpp:201-251"""
    ident = list(range(10))
    # insertion of GG between reference bases 4 | 5: keyed by hb = 5, read bases 5..6; nothing equivalent to its left or right
    got = host_window(REF10, [b"ACGTCGGATGCA"], [[0, 1, 2, 3, 4, -6, -6, 5, 6, 7, 8, 9]])
    assert got == {"kept": [{"index": 0, "align": "RRRRRRRRRR", "refHpos": [0, 1, 2, 3, 4, -1, -1, 5, 6, 7, 8, 9],
                             "indels": [[5, "+GG", 5, 5, 5, 6, 4, 5, 5, 7]], "snps": [[5, "*REF", 5, 5, 7, 7, 5, 5, 7, 7]]}]}
    # deletion of CA (reference bases 4..5): between read bases 3 | 4; the SNP map gets R=>D there
    got = host_window(REF10, [b"ACGTTGCA"], [[0, 1, 2, 3, 6, 7, 8, 9]])
    assert got == {"kept": [{"index": 0, "align": "RRRRDDRRRR", "refHpos": [0, 1, 2, 3, 6, 7, 8, 9],
                             "indels": [[4, "-CA", 4, 5, 3, 4, 3, 6, 3, 4]], "snps": [[4, "R=>D", 4, 4, 4, 4, 4, 4, 4, 4]]}]}
    # SNP C=>G at base 4: flanks one base either side; the indel map gets R=>G there
    got = host_window(REF10, [b"ACGTGATGCA"], [ident])
    assert got == {"kept": [{"index": 0, "align": "RRRRGRRRRR", "refHpos": ident,
                             "indels": [[4, "R=>G", 4, 4, 4, 4, 4, 4, 4, 4]], "snps": [[4, "C=>G", 4, 4, 4, 4, 3, 5, 3, 5]]}]}
    # overhang at the start: hpos begins with LO, the haplotype is dropped — but its SNP at base 2 still makes position 2 a variant position
    # of the window, so the reference haplotype that stays gets *REF there
    got = host_window(REF10, [REF10, b"TTACTTCATGCA"], [ident, [-1, -1] + ident])       # -1: no reference base left of the column
    assert got == {"kept": [{"index": 0, "align": "RRRRRRRRRR", "refHpos": ident,
                             "indels": [[2, "*REF", 2, 2, 2, 2, 2, 2, 2, 2]], "snps": [[2, "*REF", 2, 2, 2, 2, 2, 2, 2, 2]]}]}
    # overhang at the end: the bases behind the last reference base are RO, the haplotype is dropped; nothing else in the window
    assert host_window(REF10, [REF10 + b"GG"], [ident + [-11, -11]]) == {"kept": []}
    # a shorter copy of the reference (its trailing deletion is never recorded) is a second reference haplotype: removed
    got = host_window(REF10, [REF10, REF10[:8]], [ident, ident[:8]])
    assert [k["index"] for k in got["kept"]] == [0] and got["kept"][0]["indels"] == []
    # an N in the haplotype is an A: no variant against an A of the reference, A=>... never mentions N
    got = host_window(REF10, [b"ACGTCNTGCN"], [ident])
    assert got["kept"][0]["snps"] == [] and got["kept"][0]["align"] == "RRRRRRRRRR"
    # a block substitution is a deletion and then an insertion (rows recorded from the library, tests/golden): the deletion in front of
    # the first paired base is not recorded, the insertion is keyed behind the deleted bases and the haplotype stays
    R, L = b"GTCAGTCAGTTGCA", b"ACGTACGTACGGTCA"
    got = host_window(b"A" * 8 + R, [b"C" * 8 + R], [[-9] * 8 + list(range(8, 22))])
    assert got["kept"][0]["refHpos"] == [-1] * 8 + list(range(8, 22)) and got["kept"][0]["align"] == "D" * 8 + "R" * 14
    assert got["kept"][0]["indels"] == [[8, "+CCCCCCCC", 8, 8, 0, 7, 7, 8, 0, 8]]
    # in the middle: deletion of 10 keyed 15 between read bases 14 | 15, then the insertion keyed 25 on read bases 15..22
    got = host_window(L + b"AGAGAGAGAG" + R, [L + b"CTCTCTCT" + R], [list(range(15)) + [-26] * 8 + list(range(25, 39))])
    ind = {v[0]: v[1:6] for v in got["kept"][0]["indels"]}
    assert ind[15] == ["-AGAGAGAGAG", 15, 24, 14, 15] and ind[25] == ["+CTCTCTCT", 25, 25, 15, 22]
    # at the very end the library writes the insertion first: the deletion behind the last haplotype base is never reached
    got = host_window(L + b"A" * 8, [L + b"C" * 8], [list(range(15)) + [-16] * 8])
    assert [v[:2] for v in got["kept"][0]["indels"]] == [[15, "+CCCCCCCC"]] and got["kept"][0]["refHpos"][15:] == [-1] * 8
    bad = host_window(REF10, [b"ACG"], [[2, 1, 0]])
    assert "throw" in bad and "increase" in bad["throw"]


# ---- parser, tool, docs --------------------------------------------------------------------------------------------------------------------

def fixture_json(path, indices):
    lib = hostlib.load()
    lib.ddh_fixture_json.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.c_int, C.c_char_p, C.c_int]
    buf = C.create_string_buffer(1 << 20)
    assert lib.ddh_fixture_json(str(path).encode(), (C.c_int * len(indices))(*indices), len(indices), buf, len(buf)) > 0
    return json.loads(buf.value.decode())


def test_shared_parser_accepts_the_reference_record(tmp_path):
    f = tmp_path / "in.txt"
    f.write_text("W 3 100 109\nR ACGTCATGCA\nH ACGTCATGCA\nH ACGTTGCA\nW 4 200 209\nH ACGT\nV I 1 *REF 1 1 1 1 1 1 1 1\n")
    got = fixture_json(f, [3, 4])
    assert got[0] == [3, 100, 109, [["ACGTCATGCA", []], ["ACGTTGCA", []]], "ACGTCATGCA"]
    assert got[1] == [4, 200, 209, [["ACGT", [["I", 1, "*REF", 1, 1, 1, 1, 1, 1, 1, 1]]]]]            # no R record: as before
    f.write_text("W 3 100 109\nR\n")
    assert "line 2" in fixture_json(f, [3])["throw"]


def run_tool(*args):
    subprocess.check_call(["make", "-s", "-C", HOST])
    import torch
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return subprocess.run([os.path.join(HOST, "dindel_hapalign"), *args], env=env, capture_output=True, text=True)


def test_tool_lists_its_options_and_names_the_line_of_an_input_error(tmp_path):
    r = run_tool("--help")
    assert r.returncode == 0
    for opt in ("--hapFile", "--outputFile", "--device", "--batchWindows", "--quiet"):
        assert opt in r.stdout
    assert run_tool().returncode == 2 and run_tool("--hapFile").returncode == 2
    f, out = tmp_path / "in.txt", str(tmp_path / "out.txt")
    f.write_text("# candidates\nW 1 100 109\nH ACGTCATGCA\nW 2 200 209\nR ACGT\nH ACGT\n")
    r = run_tool("--hapFile", str(f), "--outputFile", out, "--quiet")
    assert r.returncode == 1 and "window 1 has no R record" in r.stderr and "line 2" in r.stderr
    # a later window without its R record is found before anything is written
    f.write_text("W 1 100 109\nR ACGTCATGCA\nH ACGTCATGCA\nW 2 200 209\nH ACGT\n")
    r = run_tool("--hapFile", str(f), "--outputFile", out, "--quiet", "--batchWindows", "1")
    assert r.returncode == 1 and "window 2 has no R record" in r.stderr and "line 4" in r.stderr and not os.path.exists(out)
    f.write_text("W 1 100 109\nR ACGTCATGCA\nH ACGTCATGCA\nX what\n")
    r = run_tool("--hapFile", str(f), "--outputFile", out, "--quiet")
    assert r.returncode == 1 and "Unknown record in line 4" in r.stderr
    r = run_tool("--hapFile", str(tmp_path / "none.txt"), "--outputFile", out)
    assert r.returncode == 1 and "Cannot open haplotype file" in r.stderr


DUMP_HARNESS = r'''
#include <algorithm>
#include <cctype>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>
struct RefHaplotype { std::string seq; };                         // the member the block touches (Haplotype.hpp:40-312)
static int dumpWindowIndex;
static std::string genome = "ttacgtcatgcaggacgtcatgcatt";
static std::string getRefSeq(unsigned a, unsigned b) { return genome.substr(a - 1, b - a + 1); }      // 1-based, inclusive: DInDel.cpp:1461
static void getHaplotypes(std::vector<RefHaplotype> &haps, unsigned leftPos, unsigned rightPos)
{
%s
}
int main()
{
    std::vector<RefHaplotype> haps(2);
    haps[0].seq = "ACGTCATGCA"; haps[1].seq = "ACGTTGCA";
    dumpWindowIndex = 7; getHaplotypes(haps, 2, 11);
    haps.resize(1);
    dumpWindowIndex = 9; getHaplotypes(haps, 14, 23);
    return 0;
}
'''


def test_candidate_dump_block_of_the_integration_guide_compiles_and_is_read_back(tmp_path):
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```cpp\n(.*?)\n```", text, re.S) if "DINDEL_DUMP_CANDIDATES" in b]
    assert len(blocks) == 1
    assert "<!-- compile-test" not in text[text.index(blocks[0]) - 200:text.index(blocks[0])]
    src = tmp_path / "dump.cpp"
    src.write_text(DUMP_HARNESS % blocks[0])
    exe = str(tmp_path / "dump")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", str(src), "-o", exe])
    out = tmp_path / "cands.txt"
    subprocess.check_call([exe], env=dict(os.environ, DINDEL_DUMP_CANDIDATES=str(out)))
    assert out.read_text() == "W 7 2 11\nR ACGTCATGCA\nH ACGTCATGCA\nH ACGTTGCA\nW 9 14 23\nR ACGTCATGCA\nH ACGTCATGCA\n"
    got = fixture_json(out, [7, 9])
    assert got[0] == [7, 2, 11, [["ACGTCATGCA", []], ["ACGTTGCA", []]], "ACGTCATGCA"] and got[1][4] == "ACGTCATGCA"


def test_reference_citations_of_the_new_files_point_inside_the_files():
    nlines = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_line_counts.json")))["nlines"]
    pat = re.compile(r"((?:python/)?[A-Za-z][A-Za-z0-9_]*\.(?:cpp|hpp|py|h))`?:(\d+)(?:-(\d+))?")
    n = 0
    for rel in ("dindel_tgi_amd/csrc/hapalign_kernel.hip", "dindel_tgi_amd/csrc/hapalign_kernel.h", "dindel_tgi_amd/csrc/align_host.cpp",
                "dindel_tgi_amd/host/align_haplotypes.hpp", "dindel_tgi_amd/host/align_haplotypes.cpp", "dindel_tgi_amd/host/dindel_hapalign.cpp",
                "dindel_tgi_amd/hapalign.py", "tests/_hapalign_oracle.py", "tests/golden/make_hapalign_fixtures.py", "tools/hapalign_bench.py"):
        for m in pat.finditer(open(os.path.join(ROOT, rel)).read()):
            name, a, b = m.group(1), int(m.group(2)), int(m.group(3) or m.group(2))
            if name in nlines:
                n += 1
                assert 1 <= a <= b <= nlines[name], (rel, m.group(0), nlines[name])
    assert n >= 15, n
