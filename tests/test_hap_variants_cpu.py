"""CPU-side checks of the variants kernel's surroundings and of dindel_gpu --ref's command line: the header additions, the validation
of the new entries (no launch is reached), the kernel's host twin (hapVariantsHost) with the records-to-Haplotype step against the
string walk it replaces (convertHaplotypeAlignment + finishWindowHaplotypes), the tools' options, and the citations of the new files."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from dindel_tgi_amd import capi, hapalign
from tests import _bamwriter as bw
from tests import _hap_variant_cases as hv
from tests.test_glf_vcf_cpu import write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dindel_tgi_amd", "host")


def _env():
    env = dict(os.environ)
    try:
        import torch
        env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    except ImportError:
        pass
    return env


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------

def test_header_compiles_as_c99_and_layout_agrees_with_ctypes(lib, tmp_path):
    assert lib.dd_abi_version() == 13                     # new symbols only: the ABI number does not move
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dindel_hmm.h"\n'
                   'int main(void) { dd_hap_variant v; dd_hap_variants_summary s; (void)v; (void)s;\n'
                   ' printf("%d %d %d %d %d %d %d %d %d\\n", (int)sizeof(dd_hap_variant), (int)offsetof(dd_hap_variant, kind), (int)offsetof(dd_hap_variant, key),\n'
                   '  (int)offsetof(dd_hap_variant, len), (int)offsetof(dd_hap_variant, start_read), (int)offsetof(dd_hap_variant, left_flank_hap),\n'
                   '  (int)offsetof(dd_hap_variant, right_flank_hap), (int)offsetof(dd_hap_variant, left_flank_read), (int)offsetof(dd_hap_variant, right_flank_read));\n'
                   ' printf("%d %d %d %d %d\\n", (int)sizeof(dd_hap_variants_summary), (int)offsetof(dd_hap_variants_summary, n_variants),\n'
                   '  (int)offsetof(dd_hap_variants_summary, first_base), (int)offsetof(dd_hap_variants_summary, last_base), (int)offsetof(dd_hap_variants_summary, flags));\n'
                   ' printf("%d %d %d %d %d %d %d %d\\n", DD_ALIGN_EVENT_INS, DD_ALIGN_EVENT_DEL, DD_HAP_VARIANT_SNP, DD_HAP_VARIANT_DEL_UNSEEN,\n'
                   '  DD_HAP_VARIANTS_LO_FIRST, DD_HAP_VARIANTS_RO_LAST, DD_HAP_VARIANTS_HOST, DD_HAP_VARIANTS_MAX_CAP);\n'
                   ' return 0; }\n')
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    l1, l2, l3 = subprocess.check_output([exe]).decode().split("\n")[:3]
    V, S = capi.dd_hap_variant, capi.dd_hap_variants_summary
    assert [int(x) for x in l1.split()] == [C.sizeof(V)] + [getattr(V, f).offset for f in hapalign.VARIANT_FIELDS] == [16, 0, 2, 4, 6, 8, 10, 12, 14]
    assert [int(x) for x in l2.split()] == [C.sizeof(S)] + [getattr(S, f).offset for f in hapalign.SUMMARY_FIELDS] == [16, 0, 4, 8, 12]
    assert [int(x) for x in l3.split()] == [capi.DD_ALIGN_EVENT_INS, capi.DD_ALIGN_EVENT_DEL, capi.DD_HAP_VARIANT_SNP, capi.DD_HAP_VARIANT_DEL_UNSEEN,
                                            capi.DD_HAP_VARIANTS_LO_FIRST, capi.DD_HAP_VARIANTS_RO_LAST, capi.DD_HAP_VARIANTS_HOST, capi.DD_HAP_VARIANTS_MAX_CAP]
    assert len({capi.DD_ALIGN_EVENT_INS, capi.DD_ALIGN_EVENT_DEL, capi.DD_HAP_VARIANT_SNP, capi.DD_HAP_VARIANT_DEL_UNSEEN}) == 4


def test_host_entry_returns_every_validation_error(lib):
    import torch
    good = hapalign.pack([b"ACGTACGT", b"TTGCA"], [b"ACGTCGT", b"TTGGCA", b"ACGT"], [0, 1, 0])
    INV = capi.DD_ERR_INVALID
    n, nb = 3, int(good["hap_off"][-1])
    out = {"score": np.zeros(n, np.int32), "status": np.zeros(n, np.int32), "ref_pos": np.zeros(nb, np.int16), "summary": np.zeros((n, 4), np.int32),
           "variants": np.zeros((n, 4, 8), np.int16)}

    def call(a=good, cap=4, break_=None, result=None, summary=True, variants=True, ref_pos=True):
        b = hapalign.host_batch(a)
        if break_:
            break_(b)
        r = capi.dd_align_result(out["score"].ctypes.data, out["status"].ctypes.data, out["ref_pos"].ctypes.data if ref_pos else None)
        if result:
            result(r)
        return lib.dd_align_haplotypes_variants(C.byref(b), C.byref(r), out["summary"].ctypes.data if summary else None,
                                                out["variants"].ctypes.data if variants else None, cap, 0)
    assert lib.dd_align_haplotypes_variants(None, None, None, None, 4, 0) == INV

    def changed(key, idx, val):
        a = {k: v.copy() for k, v in good.items()}
        a[key][idx] = val
        return a
    for a, what in ((changed("ref_off", 0, 1), "ref_off does not start at 0"), (changed("hap_off", 0, 2), "hap_off does not start at 0"),
                    (changed("ref_off", 1, 20), "ref_off decreases"), (changed("hap_off", 2, 3), "hap_off decreases"),
                    (changed("pair_ref", 1, 2), "pair_ref out of range"), (changed("pair_ref", 2, -1), "pair_ref out of range")):
        assert call(a) == INV and what in capi.last_error(), (what, capi.last_error())
    for field in ("ref_off", "ref_seq", "pair_ref", "hap_off", "hap_seq"):
        assert call(break_=lambda b, f=field: setattr(b, f, None)) == INV and "null" in capi.last_error(), field
    assert call(break_=lambda b: setattr(b, "n_pairs", -1)) == INV
    for field in ("score", "status"):
        assert call(result=lambda r, f=field: setattr(r, f, None)) == INV and "null" in capi.last_error(), field
    assert call(summary=False) == INV and "null summary or variants" in capi.last_error()
    assert call(variants=False) == INV and "null summary or variants" in capi.last_error()
    for cap in (0, -1, capi.DD_HAP_VARIANTS_MAX_CAP + 1):
        assert call(cap=cap) == INV and "cap outside" in capi.last_error(), cap
    b = hapalign.host_batch(good)
    assert lib.dd_align_haplotypes_variants(C.byref(b), None, out["summary"].ctypes.data, out["variants"].ctypes.data, 4, 0) == INV
    # the well-formed batch gets as far as the device, with and without room for the slice
    for ref_pos in (True, False):
        rc = call(ref_pos=ref_pos)
        if not torch.cuda.is_available():
            assert rc == capi.DD_ERR_NO_DEVICE and "no CPU fallback" in capi.last_error()


def test_device_entry_validates_before_any_launch(lib):
    """Run on a thread of its own: the library keeps "this thread's last alignment launch" per thread, and the last check needs a thread
    that has launched none, whatever ran before in this process."""
    import threading
    failures = []

    def body():
        try:
            _device_entry_checks(lib)
        except BaseException as e:                           # noqa: BLE001  (handed to the test's thread)
            failures.append(e)
    t = threading.Thread(target=body)
    t.start()
    t.join()
    if failures:
        raise failures[0]


def _device_entry_checks(lib):
    b, r = capi.dd_align_batch(), capi.dd_align_result()
    b.n_refs, b.n_pairs = 1, 1
    for f in ("ref_off", "ref_seq", "pair_ref", "hap_off", "hap_seq"):
        setattr(b, f, 4096)                                   # never dereferenced on the host
    for f in ("score", "status", "ref_pos"):
        setattr(r, f, 4096)
    fn, INV = lib.dd_hap_variants_device, capi.DD_ERR_INVALID
    assert fn(None, C.byref(r), 4096, 4096, 4, None) == INV and fn(C.byref(b), None, 4096, 4096, 4, None) == INV
    for cap in (0, capi.DD_HAP_VARIANTS_MAX_CAP + 1):
        assert fn(C.byref(b), C.byref(r), 4096, 4096, cap, None) == INV and "cap outside" in capi.last_error()
    assert fn(C.byref(b), C.byref(r), None, 4096, 4, None) == INV and "null array" in capi.last_error()
    assert fn(C.byref(b), C.byref(r), 4096, None, 4, None) == INV and "null array" in capi.last_error()
    assert fn(C.byref(b), C.byref(r), 4096, 4100, 4, None) == INV and "8-byte aligned" in capi.last_error()
    for f in ("ref_seq", "hap_seq"):
        keep = getattr(b, f)
        setattr(b, f, None)
        assert fn(C.byref(b), C.byref(r), 4096, 4096, 4, None) == INV and "null array" in capi.last_error(), f
        setattr(b, f, keep)
    r.ref_pos = None
    assert fn(C.byref(b), C.byref(r), 4096, 4096, 4, None) == INV and "null array" in capi.last_error()
    r.ref_pos = 4096
    b.n_pairs = -1
    assert fn(C.byref(b), C.byref(r), 4096, 4096, 4, None) == INV and "negative count" in capi.last_error()
    b.n_pairs = 1
    # no alignment launch of this thread to run behind: refused before anything is enqueued
    assert fn(C.byref(b), C.byref(r), 4096, 4096, 4, None) == INV and "no alignment launch" in capi.last_error()
    b.n_pairs = 0
    assert fn(C.byref(b), C.byref(r), 4096, 4096, 4, None) == 0
    out = (C.c_int64 * 4)()
    lib.dd_hap_variants_last_launch(C.byref(out))             # nothing launched: the record of no launch
    assert list(out) == [0, 0, 0, 0]


# ---- the twin against the string walk ----------------------------------------------------------------------------------------------------

def test_one_deletion_by_hand():
    """CAAAAT against CAAAT, the deletion at the front of the run (SeqAn's placement): erasing any one of the four A gives the same string, so
    the loops of getFlankingCoordinatesBetter leave leftFlankHap = 0 (sh - 1), rightFlankHap = 4 + 1 (the last x < size - l is 4);
    leftFlankRead = 0 - (1 - 0) + 1 = 0, rightFlankRead = 0 + 1 + (5 - 1 - 1) = 4."""
    summary, variants, out = hv.twin_window(b"CAAAAT", [b"CAAAT"], [[0, 2, 3, 4, 5]])
    assert summary.tolist() == [[1, 0, 6, 0]]
    assert variants[0, 0].tolist() == [capi.DD_ALIGN_EVENT_DEL, 1, 1, 0, 0, 5, 0, 4] and not variants[0, 1:].any()
    assert out["records"] == out["strings"] and out["records"]["kept"][0]["indels"] == [[1, "-A", 1, 1, 0, 1, 0, 5, 0, 4]]


def test_twin_and_records_equal_the_string_walk_on_every_case():
    cases = hv.all_cases()
    assert len(cases) >= 337 + len(hv.HAND_ROWS) + 300
    n_host = n_records = 0
    kinds = set()
    groups = {}
    for ref, hap, pos in cases:
        summary, variants, out = hv.twin_window(ref, [hap], [pos])
        assert "throw" not in out, (ref, hap, out)
        assert out["records"] == out["strings"], (ref, hap, pos)
        n, fb, lb, flags = summary[0].tolist()
        assert [fb, lb] == out["firstLast"][0], (ref, hap)
        n_host += bool(flags & capi.DD_HAP_VARIANTS_HOST)
        n_records += n
        kinds |= set(variants[0, :min(n, hv.CAP), 0].tolist())
        assert not variants[0, min(n, hv.CAP):].any()
        # the two overhang flags are the tests of finishWindowHaplotypes: a flagged haplotype is not kept
        lo, ro = pos[0] == -1, len(pos) > 1 and pos[-1] < 0 and -1 - pos[-1] == len(ref)
        assert bool(flags & capi.DD_HAP_VARIANTS_LO_FIRST) == lo and bool(flags & capi.DD_HAP_VARIANTS_RO_LAST) == ro
        assert (len(out["records"]["kept"]) == 0) == (lo or ro)
        groups.setdefault(ref, []).append((hap, pos))
    assert kinds == {capi.DD_ALIGN_EVENT_INS, capi.DD_ALIGN_EVENT_DEL, capi.DD_HAP_VARIANT_SNP, capi.DD_HAP_VARIANT_DEL_UNSEEN} and n_records >= len(cases)     # (the generator: a variant per pair on average)
    # the condition on the generator: at most 2 % of the pairs take the host flag (and the hand-written ones that must, do)
    assert 3 <= n_host <= 0.02 * len(cases), n_host
    # haplotypes that share a reference as one window: positions collected across haplotypes, R=>D from the unrecorded deletions
    shared = {r: g for r, g in groups.items() if len(g) > 1}
    assert len(shared) >= 10
    for ref, g in shared.items():
        _, _, out = hv.twin_window(ref, [h for h, _ in g], [p for _, p in g])
        assert out["records"] == out["strings"], ref
    # a small cap: the pairs beyond it go through convertHaplotypeAlignment, the count is the true one
    for ref, hap, pos in cases[::7]:
        s16, _, _ = hv.twin_window(ref, [hap], [pos])
        s1, v1, out = hv.twin_window(ref, [hap], [pos], cap=1)
        assert s1.tolist() == s16.tolist() and out["records"] == out["strings"]


# ---- the tools ------------------------------------------------------------------------------------------------------------------------------

def test_hapalign_help_shows_the_option():
    subprocess.check_call(["make", "-s", "-C", HOST])
    r = subprocess.run([os.path.join(HOST, "dindel_hapalign"), "--help"], env=_env(), capture_output=True, text=True)
    assert r.returncode == 0 and "--hostConvert" in r.stdout


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("refmode")
    rng = np.random.default_rng(3)
    ref = "".join(rng.choice(list("ACGT"), 6000))
    fasta = str(tmp / "ref.fa")
    write_fasta(fasta, [("20", ref)])
    recs = []
    for k in range(60):
        p = int(rng.integers(2900, 3050))
        recs.append(dict(qname="q%02d" % k, flag=0, pos=p, mapq=60, cigar="100M", seq=ref[p:p + 100], qual=[30] * 100, mtid=-1, mpos=-1, isize=0, tags={}))
    recs.sort(key=lambda r: r["pos"])
    bam = str(tmp / "reads.bam")
    bw.write_bam(bam, "@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:20\tLN:6000\n", [("20", 6000)], [(0, r) for r in recs])
    vf = str(tmp / "windows.txt")
    open(vf, "w").write("20 3000 3120 3060,-%s\n" % ref[3060:3062])
    subprocess.check_call(["make", "-s", "-C", HOST])
    return dict(tmp=tmp, bam=bam, vf=vf, fasta=fasta)


def test_dindel_gpu_option_errors(sample):
    exe = os.path.join(HOST, "dindel_gpu")
    base = [exe, "--bamFile", sample["bam"], "--varFile", sample["vf"], "--outputFile", str(sample["tmp"] / "e")]
    r = subprocess.run(base, env=_env(), capture_output=True, text=True)
    assert r.returncode == 1 and "--hapFile" in r.stderr and "--ref" in r.stderr       # the exit status a missing --hapFile always gave
    r = subprocess.run(base + ["--ref", str(sample["tmp"] / "missing.fa")], env=_env(), capture_output=True, text=True)
    assert r.returncode == 1 and "Exception:" in r.stderr and "missing.fa" in r.stderr
    r = subprocess.run(base + ["--ref", sample["fasta"], "--maxHap", "0"], env=_env(), capture_output=True, text=True)
    assert r.returncode == 2 and "--maxHap" in r.stderr
    r = subprocess.run([exe, "--help"], env=_env(), capture_output=True, text=True)
    assert r.returncode == 0 and all(o in r.stdout for o in ("--ref", "--maxHap", "--skipMaxHap", "--changeINStoN", "--hostDistribution", "--hostConvert"))


def test_ref_mode_prepare_only_needs_no_gpu(sample):
    out = str(sample["tmp"] / "po")
    r = subprocess.run([os.path.join(HOST, "dindel_gpu"), "--bamFile", sample["bam"], "--varFile", sample["vf"], "--ref", sample["fasta"], "--outputFile", out,
                        "--prepareOnly", "--maxHap", "4", "--skipMaxHap", "50", "--changeINStoN", "--hostDistribution", "--hostConvert"],
                       env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "windows: 1 skipped: 0" in r.stdout
    assert open(out + ".glf.txt").read().count("\n") == 1          # the header: the run stops in front of the haplotype stage


# ---- citations --------------------------------------------------------------------------------------------------------------------------------

def test_reference_citations_of_the_new_files_point_inside_the_files():
    nlines = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_line_counts.json")))["nlines"]
    pat = re.compile(r"((?:python/)?[A-Za-z][A-Za-z0-9_]*\.(?:cpp|hpp|py|h))`?:(\d+)(?:-(\d+))?")
    bad, n = [], 0
    for rel in ("dindel_tgi_amd/csrc/hap_variants_kernel.hip", "dindel_tgi_amd/csrc/hap_variants_kernel.h", "dindel_tgi_amd/host/align_haplotypes.hpp",
                "dindel_tgi_amd/host/align_haplotypes.cpp", "dindel_tgi_amd/host/haplotypes.hpp", "dindel_tgi_amd/host/dindel_gpu.cpp",
                "tests/test_ref_mode_driver_gpu.py", "tests/test_hap_variants_cpu.py", "tools/hapstage_bench.py"):
        for m in pat.finditer(open(os.path.join(ROOT, rel)).read()):
            name, a, b = m.group(1), int(m.group(2)), int(m.group(3) or m.group(2))
            if name not in nlines:
                continue
            n += 1
            if not (1 <= a <= b <= nlines[name]):
                bad.append((rel, m.group(0), nlines[name]))
    assert n > 20, n
    assert not bad, bad
