"""CPU-side checks of candidate discovery (getCIGARindels / realignCandidates): the header additions and the validation of the event
entries (no launch is reached), the event rules on the host against the gapped rows of the reference's own SeqAn
(tests/golden/hapalign_seqan.json), the CIGAR walk, the library histograms, the variant lines and the three flows of the tool with
the checker's alignments injected through the library's hook, and the tool's command line."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from dindel_tgi_amd import capi, hapalign, hostlib
from tests import _bamwriter, _candidates_cases as cases, _candidates_oracle as cand, _hapalign_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = json.load(open(os.path.join(ROOT, "tests", "golden", "hapalign_seqan.json")))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------

def test_header_additions_compile_as_c99_and_agree_with_ctypes(lib, tmp_path):
    assert lib.dd_abi_version() == 13                     # new symbols only
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dindel_hmm.h"\n'
                   'int main(void) { dd_align_events e; (void)e;\n'
                   ' printf("%d %d %d %d %d\\n", (int)sizeof(dd_align_events), (int)offsetof(dd_align_events, kind), (int)offsetof(dd_align_events, ref),\n'
                   '  (int)offsetof(dd_align_events, len), (int)offsetof(dd_align_events, hap));\n'
                   ' printf("%d %d %d %d\\n", DD_ALIGN_EVENT_INS, DD_ALIGN_EVENT_DEL, DD_ALIGN_EVENTS_MAX_CAP, DD_ALIGN_EVENTS_LOG_FIELDS);\n'
                   ' return (int)(sizeof(&dd_align_events_device) + sizeof(&dd_align_haplotypes_events) + sizeof(&dd_align_events_last_launch)) == 0; }\n')
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    l1, l2 = subprocess.check_output([exe]).decode().split("\n")[:2]
    E = capi.dd_align_events
    assert [int(x) for x in l1.split()] == [C.sizeof(E), E.kind.offset, E.ref.offset, E.len.offset, E.hap.offset] == [8, 0, 2, 4, 6]
    assert [int(x) for x in l2.split()] == [capi.DD_ALIGN_EVENT_INS, capi.DD_ALIGN_EVENT_DEL, capi.DD_ALIGN_EVENTS_MAX_CAP, len(capi.ALIGN_EVENTS_LOG_FIELDS)]


def _events_call(lib, a, cap=4, break_=None, result=None, n_events=True, events=True):
    b = hapalign.host_batch(a)
    if break_:
        break_(b)
    n = max(len(a["hap_off"]) - 1, 1)
    out = {"score": np.zeros(n, np.int32), "status": np.zeros(n, np.int32), "n": np.zeros(n, np.int32), "ev": np.zeros((n, max(cap, 1), 4), np.int16)}
    r = capi.dd_align_result(out["score"].ctypes.data, out["status"].ctypes.data, None)
    if result:
        result(r)
    return lib.dd_align_haplotypes_events(C.byref(b), C.byref(r), out["n"].ctypes.data if n_events else None, out["ev"].ctypes.data if events else None, cap, 0)


def test_every_validation_error_of_the_event_entries(lib):
    import torch
    good = hapalign.pack([b"ACGTACGT", b"TTGCA"], [b"ACGTCGT", b"TTGGCA", b"ACGT"], [0, 1, 0])
    INV = capi.DD_ERR_INVALID
    assert lib.dd_align_haplotypes_events(None, None, None, None, 4, 0) == INV

    def changed(key, idx, val):
        a = {k: v.copy() for k, v in good.items()}
        a[key][idx] = val
        return a
    for a, what in ((changed("ref_off", 0, 1), "ref_off does not start at 0"), (changed("hap_off", 0, 2), "hap_off does not start at 0"),
                    (changed("ref_off", 1, 20), "ref_off decreases"), (changed("hap_off", 2, 3), "hap_off decreases"),
                    (changed("pair_ref", 1, 2), "pair_ref out of range"), (changed("pair_ref", 2, -1), "pair_ref out of range")):
        assert _events_call(lib, a) == INV and what in capi.last_error(), (what, capi.last_error())
    for field in ("ref_off", "ref_seq", "pair_ref", "hap_off", "hap_seq"):
        assert _events_call(lib, good, break_=lambda b, f=field: setattr(b, f, None)) == INV and "null" in capi.last_error(), field
    assert _events_call(lib, good, break_=lambda b: setattr(b, "n_pairs", -1)) == INV
    for field in ("score", "status"):
        assert _events_call(lib, good, result=lambda r, f=field: setattr(r, f, None)) == INV and "null" in capi.last_error(), field
    assert _events_call(lib, good, n_events=False) == INV and "n_events" in capi.last_error()
    assert _events_call(lib, good, events=False) == INV and "events" in capi.last_error()
    for cap in (0, -1, capi.DD_ALIGN_EVENTS_MAX_CAP + 1):
        assert _events_call(lib, good, cap=cap) == INV and "events_cap" in capi.last_error(), cap
    # a well-formed call with no slice asked for (ref_pos NULL) gets as far as the device
    rc = _events_call(lib, good)
    if not torch.cuda.is_available():
        assert rc == capi.DD_ERR_NO_DEVICE and "no CPU fallback" in capi.last_error()


def test_device_event_entry_validates_before_any_launch(lib):
    b, r = capi.dd_align_batch(), capi.dd_align_result()
    b.n_refs, b.n_pairs = 1, 1
    for f in ("ref_off", "ref_seq", "pair_ref", "hap_off", "hap_seq"):
        setattr(b, f, 4096)                                   # never dereferenced on the host
    for f in ("score", "status", "ref_pos"):
        setattr(r, f, 4096)
    fn, INV = lib.dd_align_events_device, capi.DD_ERR_INVALID
    assert fn(None, C.byref(r), 4096, 4096, 4, None) == INV
    assert fn(C.byref(b), None, 4096, 4096, 4, None) == INV
    assert fn(C.byref(b), C.byref(r), 4096, 4096, 0, None) == INV and "events_cap" in capi.last_error()
    assert fn(C.byref(b), C.byref(r), 4096, 4096, capi.DD_ALIGN_EVENTS_MAX_CAP + 1, None) == INV
    assert fn(C.byref(b), C.byref(r), None, 4096, 4, None) == INV and "null array" in capi.last_error()
    assert fn(C.byref(b), C.byref(r), 4096, None, 4, None) == INV and "null array" in capi.last_error()
    assert fn(C.byref(b), C.byref(r), 4096, 4098, 4, None) == INV and "aligned" in capi.last_error()
    r.ref_pos = None
    assert fn(C.byref(b), C.byref(r), 4096, 4096, 4, None) == INV and "null array" in capi.last_error()
    r.ref_pos = 4096
    # this thread has launched no alignment whose workspace header could hold the counter
    assert fn(C.byref(b), C.byref(r), 4096, 4096, 4, None) == INV and "no alignment launch" in capi.last_error()
    b.n_pairs = 0
    assert fn(C.byref(b), C.byref(r), 4096, 4096, 4, None) == capi.DD_SUCCESS
    out = (C.c_int64 * 4)()
    lib.dd_align_events_last_launch(C.byref(out))            # nothing launched: readable, no device touched


# ---- the event rules ----------------------------------------------------------------------------------------------------------------------

def host_events(pos, ref_len, cap=64):
    lib = hostlib.load()
    lib.ddh_alignment_events.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    pos = np.ascontiguousarray(pos, np.int16)
    out = np.zeros((cap, 4), np.int16)
    n = lib.ddh_alignment_events(pos.ctypes.data if pos.size else None, len(pos), ref_len, out.ctypes.data, cap)
    assert 0 <= n <= cap
    return [tuple(int(v) for v in row) for row in out[:n]]


def test_events_from_slices_equal_events_from_seqan_rows_on_every_fixture():
    """the slices are the checker's, the rows SeqAn's own: this pins the event rules of dd_align_events"""
    kinds = set()
    for c in FIXTURES:
        ref, hap = c["ref"].encode("latin-1"), c["hap"].encode("latin-1")
        want = cand.events_from_rows(c["row0"], c["row1"])
        got = host_events(orc.align(ref, hap)[3], len(ref))
        assert got == want, (c, got, want)
        kinds.update(k for k, _, _, _ in want)
    assert kinds == {cand.INS, cand.DEL}


def test_event_rules_on_hand_derived_slices():
    G = lambda n: -1 - n
    I, D = capi.DD_ALIGN_EVENT_INS, capi.DD_ALIGN_EVENT_DEL
    assert host_events([0, 1, 2, 3], 4) == []
    assert host_events([G(0), G(0), 0, 1], 2) == []                             # leading insertion: LO
    assert host_events([2, 3, 4], 5) == []                                      # deletion in front of the first paired base; trailing deletion
    assert host_events([0, 1, G(2), G(2)], 2) == []                             # trailing insertion at the reference's end: RO
    assert host_events([0, 1, G(2), G(2), 2], 3) == [(I, 2, 2, 2)]
    assert host_events([0, 1, 4, 5], 6) == [(D, 2, 2, 2)]
    assert host_events([0, G(3), G(3), 3], 4) == [(D, 1, 2, 1), (I, 3, 2, 1)]   # block substitution: deletion, then insertion
    assert host_events([0, G(1), G(1), 3], 4) == [(I, 1, 2, 1), (D, 1, 2, 3)]   # ... and the order of the matrix edge
    assert host_events([G(0), 2, 3], 4) == []                                   # LO, then a deletion before any paired base
    assert host_events([G(2), 2, 3], 4) == [(I, 2, 1, 0)]                       # not the leading run: reference bases lie in front of it
    assert host_events([], 3) == []


# ---- the CIGAR walk -----------------------------------------------------------------------------------------------------------------------

def lib_cigar_indels(pos, cigar, seq):
    lib = hostlib.load()
    lib.ddh_cigar_indels_json.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int]
    rec, _ = _bamwriter.encode_record(0, dict(qname="q", flag=0, pos=pos, cigar=cigar, seq=seq, qual=[30] * len(seq)))
    out = C.create_string_buffer(1 << 16)
    assert lib.ddh_cigar_indels_json(rec[4:], len(rec) - 4, out, len(out)) > 0
    return json.loads(out.value.decode())


@pytest.mark.parametrize("pos,cigar,seq", [
    (100, "10M", "ACGTACGTAC"), (100, "4M2I4M", "ACGTNNACGT"), (7, "3M4D3M", "ACGTAC"), (50, "2S3M1I2M3N2M2D1M2S", "TTACGRACGTAGG"),
    (50, "3H2S4M1I1D3M1S2H", "GGACGTWCCAT"), (9, "2M1I1D1I2M", "ACMKGT"), (0, "1I5M", "=ACGTA"), (3, "5M1I", "ACGTAY")])
def test_cigar_indels_equal_the_restatement(pos, cigar, seq):
    got = lib_cigar_indels(pos, cigar, seq)
    assert "throw" not in got and [tuple(x) for x in got["indels"]] == cand.cigar_indels(pos, cigar, seq)


@pytest.mark.parametrize("cigar,seq", [("3M1P3M", "ACGTAC"), ("2M2=2M", "ACGTAC"), ("1I2X", "ACG")])
def test_unknown_cigar_operation_throws_the_reference_text(cigar, seq):
    got = lib_cigar_indels(10, cigar, seq)
    assert got["throw"] == "I don't know how to smoke this CIGAR"
    with pytest.raises(ValueError, match="smoke this CIGAR"):
        cand.cigar_indels(10, cigar, seq)


def test_hash_map_order_is_a_permutation_and_ignores_repeats():
    keys = [5, 100003, 7, 5, 193, 386, 7, 0, 1 << 20]
    order = cand.hash_order(keys)
    assert sorted(order) == sorted(set(keys)) and cand.hash_order(order[::-1] + keys) != [] and len(order) == 7


# ---- the flows, with the checker's alignments injected ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    return cases.bam_sample(tmp_path_factory.mktemp("cand"))


@pytest.fixture(scope="module")
def whole_run(sample, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("whole") / "o")
    assert cases.run_in_library(["--analysis", "getCIGARindels", "--bamFile", sample["bam"], "--ref", sample["fasta"], "--outputFile", out, "--quiet"]) == 0
    return out, cand.whole_file(sample["header"], sample["names"], sample["records"], sample["targets"])


def test_whole_file_variants_equal_the_restatement(whole_run):
    out, (want_variants, _) = whole_run
    got = open(out + ".variants.txt").read()
    assert got == want_variants and got.count("\n") > 20
    for line in got.split("\n")[:-1]:                         # `tid pos var ... # count ...`, one count per variant, single blanks
        left, right = line.split(" #")
        w, counts = left.split(" "), right.split(" ")
        assert w[0].startswith("chr") and int(w[1]) >= 0 and all(v[0] in "+-" for v in w[2:]) and counts[0] == "" and len(counts) - 1 == len(w) - 2


def test_written_variants_read_back_to_the_same_positions_and_variants(sample, whole_run, tmp_path):
    """The file is the input format of realignCandidates (VariantFile::getLine: `tid pos variant ... # ...`); the window-file parser behind
    ddh_window_lines_json reads another format (`tid left right pos,variant ...`) and throws at these lines, so the reading back is done
    by the tool's own reader: every canonical variant realigns to itself (the counts become 1: one line, one candidate each)."""
    out, _ = whole_run
    again = str(tmp_path / "again")
    assert cases.run_in_library(["--analysis", "realignCandidates", "--varFile", out + ".variants.txt", "--ref", sample["fasta"], "--outputFile", again, "--quiet"]) == 0
    first = [l.split(" #")[0] for l in open(out + ".variants.txt")]
    second = open(again + ".variants.txt").read().split("\n")[:-1]
    assert [l.split(" #")[0] for l in second] == first and all(set(l.split(" #")[1].split()) == {"1"} for l in second)
    lib = hostlib.load()
    lib.ddh_window_lines_json.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int]
    buf = C.create_string_buffer(1 << 20)
    assert lib.ddh_window_lines_json((out + ".variants.txt").encode(), 0, buf, len(buf)) > 0
    assert json.loads(buf.value.decode()).get("throw") == "Cannot read left boundary of region."


def test_library_histograms_equal_the_restatement_and_parse(sample, whole_run):
    out, (_, want_libraries) = whole_run
    got = open(out + ".libraries.txt").read()
    assert got == want_libraries
    names = [l.split()[1] for l in got.split("\n") if l.startswith("#LIB")]
    assert names == sorted(names) and set(names) == {"dindel_default", "libOne", "libTwo"}
    # libTwo: 150 ... 152, the 300s of records without a library behind it, and a few 30,000s beyond ten medians, which stay out of
    # mean and variance: the table ends far in front of them
    two = got.split("#LIB libTwo\n")[1].split("#LIB")[0].split("\n")[:-1]
    assert 150 < len(two) < 3000 and two[0].startswith("0 ") and [int(l.split()[0]) for l in two] == list(range(len(two)))
    lib = hostlib.load()
    lib.ddh_parse_inputs_json.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int]
    buf = C.create_string_buffer(1 << 16)
    assert lib.ddh_parse_inputs_json(b"", 0, (out + ".libraries.txt").encode(), buf, len(buf)) > 0
    parsed = json.loads(buf.value.decode())
    assert "throw" not in parsed and set(parsed["libraries"]) == set(names) | {"single_end"}


def test_host_convert_and_host_events_write_the_same_file(sample, whole_run, tmp_path):
    out, _ = whole_run
    other = str(tmp_path / "h")
    assert cases.run_in_library(["--analysis", "getCIGARindels", "--bamFile", sample["bam"], "--ref", sample["fasta"], "--outputFile", other, "--quiet",
                                 "--hostConvert", "--batchCandidates", "7"]) == 0
    assert open(other + ".variants.txt").read() == open(out + ".variants.txt").read()
    assert open(other + ".libraries.txt").read() == open(out + ".libraries.txt").read()


def test_region_run_over_two_files(sample, tmp_path):
    second = cases.bam_sample(tmp_path, name="second", seed=12, n_reads=120)
    lst = tmp_path / "bams.txt"
    lst.write_text(sample["bam"] + "\n" + second["bam"] + "\n")
    out = str(tmp_path / "region.txt")
    assert cases.run_in_library(["--analysis", "getCIGARindels", "--bamFiles", str(lst), "--tid", "chrA", "--region", "500-2,000", "--ref", sample["fasta"],
                                 "--outputFile", out, "--quiet"]) == 0
    table = cand.Table()
    for s in (sample, second):
        for tid, r in s["records"]:
            if tid == 0 and r["pos"] < 2000 and r["pos"] + _bamwriter.ref_len(_bamwriter.parse_cigar(r["cigar"])) > 500:
                for c in cand.cigar_indels(r["pos"], r["cigar"], r["seq"]):
                    table.add(*c)
    want = cand.output_indels("chrA", table, sample["targets"]["chrA"])
    assert open(out).read() == want and want.count("\n") >= 5


@pytest.mark.parametrize("one_based", [False, True])
def test_realign_candidates_near_the_edges_of_a_target(tmp_path, one_based):
    """candidates within 100 bases of either end of a target, beyond its end, on an unknown target, a 34-base one (the wider window) and
    one too long for the device: tool = restatement"""
    import random
    rng = random.Random(21)
    t = cases.rand_seq(rng, 150) + "AAAAAAA" + cases.rand_seq(rng, 200) + "ACACACAC" + cases.rand_seq(rng, 90)
    fasta = str(tmp_path / "e.fa")
    cases.write_fasta(fasta, [("e", t), ("f", cases.rand_seq(rng, 5000))])
    cands = [(3, 2, "GG"), (40, -3, ""), (99, 1, "T"), (101, -2, ""), (152, -1, ""), (154, 1, "A"), (360, -2, ""), (362, 2, "AC"), (len(t) - 30, -4, ""),
             (len(t) - 2, 3, "CCC"), (len(t) - 2, -5, ""), (len(t) + 50, 1, "A"), (len(t) + 150, -1, ""), (200, 34, cases.rand_seq(rng, 34)), (200, -33, "")]
    text = cases.candidate_file_text("e", cands, t + "N" * 400, one_based)
    text += "nowhere 10 +A # 1\n" + "f 2500 +%s # 2\n" % cases.rand_seq(rng, 1400) + "f 2400 +C -%s A=>C # 1 1 1\n" % "G"
    vf = tmp_path / "in.txt"
    vf.write_text(text)
    out = str(tmp_path / "o")
    args = ["--analysis", "realignCandidates", "--varFile", str(vf), "--ref", fasta, "--outputFile", out, "--quiet"] + (["--varFileIsOneBased"] if one_based else [])
    assert cases.run_in_library(args) == 0
    want = cand.realign_file(text, one_based, {"e": t, "f": open(fasta).read().split(">f\n")[1].replace("\n", ""), "nowhere": ""})
    got = open(out + ".variants.txt").read()
    assert got == want and got.count("\n") >= 8 and "nowhere" not in got
    assert cases.run_in_library(args + ["--hostConvert"]) == 0 and open(out + ".variants.txt").read() == want


# ---- the command line --------------------------------------------------------------------------------------------------------------------

def test_tool_help_and_option_errors(tmp_path):
    rc, out, _ = cases.run_tool(["--help"])
    assert rc == 0
    for opt in ("--analysis", "--bamFile", "--bamFiles", "--ref", "--outputFile", "--tid", "--region", "--varFile", "--varFileIsOneBased", "--device",
                "--batchCandidates", "--eventsCap", "--hostConvert", "--quiet", "--help"):
        assert opt in out, opt
    base = ["--ref", "r.fa", "--outputFile", str(tmp_path / "o")]
    for args, code, text in (
            (base, 1, "Error: Specify which analysis (--analysis) is required."),
            (["--analysis", "getCIGARindels", "--ref", "r.fa"], 1, "Error: One of the following options was not specified:  --ref --tid or --outputFile"),
            (["--analysis", "getCIGARindels"] + base, 1, "Error: Specify either --bamFile or --bamFiles."),
            (["--analysis", "getCIGARindels", "--bamFiles", "l.txt"] + base, 1, "Can extract the full set of indels from only BAM file at a time."),
            (["--analysis", "getCIGARindels", "--bamFile", "x.bam", "--region", "1-2"] + base, 1, "--tid must be specified if analysis==getCIGARindels and --region option is used. "),
            (["--analysis", "realignCandidates"] + base, 1, "Please specify the file with the candidate variants."),
            (["--analysis", "realignCandidates", "--varFile", str(tmp_path / "o") + ".variants.txt"] + base, 1, "outputFile is same as variant file used for input!"),
            (["--analysis", "indels"] + base, 1, "Unrecognized --analysis option."),
            (["--analysis", "realignCandidates", "--varFile", "v", "--eventsCap", "0"] + base, 2, "--eventsCap"),
            (["--analysis", "realignCandidates", "--varFile", "v", "--batchCandidates", "0"] + base, 2, "--batchCandidates")):
        rc, out, err = cases.run_tool(args)
        assert rc == code and text in err, (args, rc, err)
    rc, out, err = cases.run_tool(["--analysis"])
    assert rc == 1 and "Error parsing input options" in out
    rc, out, err = cases.run_tool(["--analysis", "realignCandidates", "--varFile", str(tmp_path / "missing"), "--ref", str(tmp_path / "none.fa"), "--outputFile", str(tmp_path / "o")])
    assert rc == 1 and out.startswith("Exception: Cannot open file ")
