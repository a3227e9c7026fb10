"""CPU-side checks of the audit of the --faster model (dd_audit_select_faster, dd_audit_shadow_faster_host, dd_audit_compare_host_faster,
dd_audit_device_faster): the second implementation of ObservationModelS (csrc/faster_shadow.h) looped on the CPU against the oracle's
restatement, bit for bit on every element the rule names; the rule with planted differences against a numpy restatement written unlike it;
the sample's rules; declarations and validation; the independence of the new sources from the two --faster kernels' text; and selection,
shadow and comparison over random batches in a stand-alone program under AddressSanitizer and UBSan.  No compute on a device here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from dindel_tgi_amd import capi, synth
from tests import _audit_cases as ac
from tests import _audit_faster_cases as fc
from tests import _path_scenarios as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dindel_tgi_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW_SOURCES = ("faster_shadow.h", "faster_shadow_host.cpp", "faster_shadow_kernel.hip", "faster_shadow_capi.cpp")
ALL = capi.DD_OPT_LONG_WINDOWS_FASTER


def has_flank(pb):
    return pb.hap_var_flank is not None and len(pb.hap_var_flank) > 0


def shadow_against_oracle(pb, p, want=None):
    """The CPU shadow of every eligible window (the long ones too) into poisoned arrays of exactly the sample's lengths: bit-equal to the
    oracle where the rule names an element, untouched elsewhere; the CPU comparison finds nothing and counts what numpy counts.
    -> the statuses of the sample's pairs."""
    want = fc.oracle(p, pb) if want is None else want
    cls = fc.faster_classes(p, pb, True)
    smp = capi.AuditSample(p, pb, pb.n_windows, win_class=cls, faster=True, options=ALL)
    assert list(smp.chosen) == list(fc.eligible_windows(pb, cls, True))
    sh = fc.poisoned_shadow(smp)
    capi.audit_shadow_faster_host(p, pb, smp, fc.result_struct(sh))
    exp, mask = fc.owned_shadow(pb, smp, want)
    fc.assert_shadow_is_the_oracles(sh, exp, mask, fc.SHADOW_POISON)
    rep = capi.audit_compare_host_faster(pb, fc.result_struct(want), smp, fc.result_struct(sh), 8)
    assert rep["n_diff"] == 0 and rep["n_pairs"] == smp.sizes.n_pairs, rep["records"]
    assert rep["compared"] == fc.expected_compared(pb, want["status"], smp.chosen, has_flank(pb))
    return exp["status"]


SCENARIOS = [(hl, L, mld) for hl in ps.FASTER_HAP_LENGTHS for L in (36, 100) for mld in (5, 11)]


def test_shadow_is_bit_equal_to_the_oracle_on_the_scenario_batches(lib):
    seen = set()
    for hl, L, mld in SCENARIOS:
        pb, index, p, want = fc.scenario(hl, L, mld)
        seen |= set(np.unique(shadow_against_oracle(pb, p, want)).tolist())
    assert seen == {capi.DD_PAIR_OK, capi.DD_PAIR_NAN, capi.DD_PAIR_HAPSIZE}     # nothing is left out silently


def test_shadow_is_bit_equal_to_the_oracle_on_the_smallest_long_shapes(lib):
    pb, p, want = fc.long_scenario()
    hl, rl = np.diff(pb.a["hap_seq_off"]), np.diff(pb.a["read_seq_off"])
    assert 767 in hl and 1025 in rl and list(fc.faster_classes(p, pb, True)) == [0, 2, 2, 0]
    st = shadow_against_oracle(pb, p, want)
    assert (st == capi.DD_PAIR_OK).all()


@pytest.mark.parametrize("mld", [5, 3])
def test_shadow_is_bit_equal_to_the_oracle_where_the_model_can_go_wrong(lib, mld):
    """tests/_audit_faster_cases.handmade_batch: reads of 3, 4 and 5 bp, haplotypes of 3 ... 7 bp (zero and one hashed k-mer; at maxLengthDel 3
    the 4-bp haplotype is computed, at 5 it is a hapSize error), junk reads (the sentinel alone), tandem repeats (more than 15 diagonals with
    equal counts), reads left and right of the window, N / lower case / IUPAC, mapping qualities on both sides of the cap, variants and
    flanks with an interval reaching below base 0."""
    pb, names = fc.handmade_batch()
    p = ps.params_for(mld, 0)
    want = fc.oracle(p, pb)
    st = shadow_against_oracle(pb, p, want)
    assert all((st == s).any() for s in (capi.DD_PAIR_OK, capi.DD_PAIR_NAN, capi.DD_PAIR_HAPSIZE))
    # the cases are what their names say
    w_of = ac.window_of_pairs(pb)
    full = np.asarray(want["status"])[:pb.n_pairs]
    assert (full[w_of == names["short reads"]] == [capi.DD_PAIR_NAN, capi.DD_PAIR_OK, capi.DD_PAIR_OK, capi.DD_PAIR_NAN]).all()
    four = full[w_of == names["hlen 4 and 5"]]
    assert (four[:3] == (capi.DD_PAIR_HAPSIZE if mld == 5 else capi.DD_PAIR_OK)).all() and (four[3:] == capi.DD_PAIR_OK).all()
    assert list(full[w_of == names["hapsize"]]) == [capi.DD_PAIR_HAPSIZE, capi.DD_PAIR_HAPSIZE if mld == 5 else capi.DD_PAIR_OK, capi.DD_PAIR_OK]
    flank = pb.hap_var_flank.reshape(-1, 3)
    assert (flank[:, 0] - p.padCover < 0).any()
    cov = np.asarray(want["var_fcov"])[:pb.var_cov_len]
    assert cov.any() and not cov.all() and np.asarray(want["var_covered"])[:pb.var_cov_len].any()
    # both sides of capMapQualFast: the table the join reads holds capped and uncapped priors
    tab = np.zeros(capi.DD_TABLE_DOUBLES)
    b = pb.ctypes_batch()
    assert lib.dd_build_tables(C.byref(p), b.qual_table, b.n_qual, b.mapq_table, b.n_mapq, tab.ctypes.data_as(capi.c_f64p)) > 0
    mq = np.array([b.mapq_table[i] for i in range(b.n_mapq)])
    capped = -10 * np.log10(1 - mq) > p.capMapQualFast
    assert capped.any() and (~capped).any()


def test_the_tandem_case_has_more_than_fifteen_tied_diagonals():
    pb, names = fc.handmade_batch()
    a = pb.a
    w = names["tandem"]
    g, q = int(a["win_hap_off"][w]), int(a["win_read_off"][w])
    hap = bytes(a["hap_seq"][a["hap_seq_off"][g]:a["hap_seq_off"][g + 1]]).decode()
    read = bytes(a["read_seq"][a["read_seq_off"][q]:a["read_seq_off"][q + 1]]).decode()
    votes = {}
    for x in range(len(read) - 3):
        for hx in range(len(hap) - 4):
            if hap[hx:hx + 4] == read[x:x + 4]:
                votes[hx - x] = votes.get(hx - x, 0) + 1
    top = max(votes.values())
    assert sum(1 for v in votes.values() if v == top) > 15


# ---- the rule ----
def compare_case():
    pb, index, p, want = fc.scenario()
    smp = capi.AuditSample(p, pb, pb.n_windows, win_class=fc.faster_classes(p, pb), faster=True)
    primary = {k: np.array(v, copy=True) for k, v in want.items()}
    shadow = ac.shadow_from(pb, smp, want)
    return pb, p, want, smp, primary, shadow


def run_compare(pb, primary, smp, shadow, cap=64, null_p=(), null_s=()):
    return capi.audit_compare_host_faster(pb, ac.result_struct(primary, null_p), smp, ac.result_struct(shadow, null_s), cap)


def shadow_index(pb, smp, k, e):
    full = {"hpos": pb.win_hpos_off, "var_covered": pb.win_varcov_off, "var_fcov": pb.win_varcov_off}.get(k, pb.win_pair_off)
    mine = {"hpos": smp.hpos_off, "var_covered": smp.varcov_off, "var_fcov": smp.varcov_off}.get(k, smp.pair_off)
    w = int(np.searchsorted(np.asarray(full), e, side="right")) - 1
    assert w in smp.chosen
    return int(mine[w]) + e - int(full[w]), w


def test_one_inverted_bit_in_each_field_on_either_side_is_reported():
    pb, p, want, smp, primary, shadow = compare_case()
    assert run_compare(pb, primary, smp, shadow)["n_diff"] == 0
    elem = ps.element_pairs(pb)
    st = np.asarray(want["status"])[:pb.n_pairs]
    in_sample = np.isin(ac.window_of_pairs(pb), smp.chosen)
    ok = np.nonzero(in_sample & (st == capi.DD_PAIR_OK))[0]
    pair = int(ok[len(ok) // 2])
    hp = np.nonzero(elem["hpos"][:pb.hpos_len] == pair)[0]
    vc = np.nonzero(np.isin(elem["var_covered"][:pb.var_cov_len], ok))[0]
    targets = [(k, pair) for k in capi.AUDIT_FIELDS[:15]] + [("hpos", int(hp[0])), ("hpos", int(hp[-1])), ("var_covered", int(vc[0])), ("var_fcov", int(vc[-1]))]
    # a thrown pair's owned fields too
    for s in fc.THROWN:
        thrown = int(np.nonzero(in_sample & (st == s))[0][0])
        targets += [(k, thrown) for k in capi.AUDIT_FIELDS[1:13]]
    for side in ("primary", "shadow"):
        for k, e in targets:
            arrs = primary if side == "primary" else shadow
            at, w = shadow_index(pb, smp, k, e)
            if side == "primary":
                at = e
            raw = arrs[k].view(np.uint8).reshape(len(arrs[k]), -1)
            raw[at, 0] ^= 0x04
            try:
                rep = run_compare(pb, primary, smp, shadow)
            finally:
                raw[at, 0] ^= 0x04
            assert rep["n_diff"] == 1 and rep["diff"][k] == 1 and sum(rep["diff"].values()) == 1, (side, k, e, rep["diff"])
            r = rep["records"][0]
            owner = int(elem[k][e]) if k in ac.PER_ELEMENT else e
            bits = int(np.asarray(want[k][e:e + 1]).view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[want[k].dtype.itemsize])[0])
            assert (r["window"], r["field"], r["pair"], r["index"]) == (w, k, owner, e), (side, k, r)
            assert (r["primary_bits"], r["shadow_bits"]) == ((bits ^ 4, bits) if side == "primary" else (bits, bits ^ 4)), (side, k, r)


def test_a_status_difference_hides_the_rest_and_unowned_elements_are_never_read():
    pb, p, want, smp, primary, shadow = compare_case()
    st = np.asarray(want["status"])[:pb.n_pairs]
    elem = ps.element_pairs(pb)
    in_sample = np.isin(ac.window_of_pairs(pb), smp.chosen)
    pair = int(np.nonzero(in_sample & (st == capi.DD_PAIR_OK))[0][3])
    primary["status"][pair] = capi.DD_PAIR_NAN
    primary["ll"][pair] += 1.0
    primary["hpos"][np.nonzero(elem["hpos"][:pb.hpos_len] == pair)[0]] ^= 1
    rep = run_compare(pb, primary, smp, shadow)
    assert rep["n_diff"] == 1 and rep["records"][0]["field"] == "status" and rep["records"][0]["pair"] == pair
    assert (rep["records"][0]["primary_bits"], rep["records"][0]["shadow_bits"]) == (capi.DD_PAIR_NAN, capi.DD_PAIR_OK)
    base = fc.expected_compared(pb, want["status"], smp.chosen, True)
    L = int((elem["hpos"][:pb.hpos_len] == pair).sum())
    assert rep["compared"]["ll"] == base["ll"] - 1 and rep["compared"]["hpos"] == base["hpos"] - L and rep["compared"]["status"] == base["status"]
    # the elements a thrown pair does not own hold different poison on the two sides: not reported (the main model's rule would read them
    # under DD_PAIR_NAN)
    pb, p, want, smp, primary, shadow = compare_case()
    thrown = np.nonzero(in_sample & np.isin(st, fc.THROWN))[0]
    assert (st[thrown] == capi.DD_PAIR_NAN).any() and (st[thrown] == capi.DD_PAIR_HAPSIZE).any()
    sh_thrown = np.array([shadow_index(pb, smp, "ll", int(e))[0] for e in thrown])
    for k in ("firstBase", "lastBase"):
        primary[k][thrown] = 0x5A5A
        shadow[k][sh_thrown] = 0x3C3C
    hp = np.nonzero(np.isin(elem["hpos"][:pb.hpos_len], thrown))[0]
    assert hp.size
    primary["hpos"][hp] = 0x5A5A
    shadow["hpos"][[shadow_index(pb, smp, "hpos", int(e))[0] for e in hp]] = 0x3C3C
    primary["onHap"][...] ^= 1                                           # never compared
    outside = np.nonzero(~in_sample)[0]
    primary["ll"][outside] = 1.0                                         # a window outside the sample
    rep = run_compare(pb, primary, smp, shadow)
    assert rep["n_diff"] == 0, rep["records"][:3]
    legacy = capi.audit_compare_host(pb, ac.result_struct(primary), smp, ac.result_struct(shadow), 4)
    assert legacy["diff"]["hpos"] > 0 and legacy["diff"]["firstBase"] > 0   # ... which is why this model has a rule of its own
    # ... while an owned element of a thrown pair is compared
    primary["offHapHMQ"][thrown[0]] ^= 1
    rep = run_compare(pb, primary, smp, shadow)
    assert rep["n_diff"] == 1 and rep["records"][0]["field"] == "offHapHMQ" and rep["records"][0]["pair"] == int(thrown[0])
    primary["offHapHMQ"][thrown[0]] ^= 1
    # NULL fields on either side are skipped, with their differences
    ok = int(np.nonzero(in_sample & (st == capi.DD_PAIR_OK))[0][0])
    primary["llOn"][ok] += 1.0
    primary["var_fcov"][...] ^= 1
    assert run_compare(pb, primary, smp, shadow)["n_diff"] > 1
    for kw in (dict(null_p=("llOn", "var_fcov")), dict(null_s=("llOn", "var_fcov")), dict(null_p=("llOn",), null_s=("var_fcov",))):
        rep = run_compare(pb, primary, smp, shadow, **kw)
        assert rep["n_diff"] == 0 and rep["compared"]["llOn"] == 0 and rep["compared"]["var_fcov"] == 0 and rep["compared"]["llOff"] > 0, kw


@pytest.mark.parametrize("cap", [0, 1, 2])
def test_a_small_record_cap_keeps_the_counts_right(cap):
    pb, p, want, smp, primary, shadow = compare_case()
    st = np.asarray(want["status"])[:pb.n_pairs]
    in_sample = np.isin(ac.window_of_pairs(pb), smp.chosen)
    ok = np.nonzero(in_sample & (st == capi.DD_PAIR_OK))[0][:5]
    primary["ll"][ok] += 1.0
    primary["lastBase"][ok[:2]] += 1
    guard = capi.audit_report_buffer(cap + 1)
    guard[...] = 0xEE
    b = pb.ctypes_batch()
    v = smp.view()
    rc = capi.load().dd_audit_compare_host_faster(C.byref(b), C.byref(ac.result_struct(primary)), C.byref(v), C.byref(ac.result_struct(shadow)),
                                                  guard.ctypes.data, cap)
    assert rc == 0
    rep = capi.audit_report(guard, cap)
    assert rep["n_diff"] == 7 and rep["diff"]["ll"] == 5 and rep["diff"]["lastBase"] == 2 and len(rep["records"]) == cap
    assert (guard[C.sizeof(capi.dd_audit_report) + cap * C.sizeof(capi.dd_audit_record):] == 0xEE).all()


# ---- the sample ----
def sample_batch():
    """Windows 0, 2, 5: ordinary (2 holds the longest ordinary haplotype, 5 the longest ordinary read); 1: a 900-bp haplotype, 4: a 1,100-bp
    read (long with the option); 3: haplotypes without reads; 6: an empty read (unsupported); 7 ... 12: ordinary and small."""
    from dindel_tgi_amd.batch import Window, ReadRec, pack
    rng = np.random.default_rng(5)
    S = ps.HAP_START
    h = [ps.rnd(rng, n) for n in (60, 900, 300, 60, 200, 80, 60)]
    reads = lambda hap, n, L=30: ps.spread_reads(rng, hap, n, L)
    ws = [Window(S, [h[0], h[0][:30] + h[0][31:]], reads(h[0], 4)),
          Window(S, [h[1]], reads(h[1], 2)),
          Window(S, [h[2]], reads(h[2], 3)),
          Window(S, [h[3]], []),
          Window(S, [h[4]], reads(h[4], 1, 1100)),
          Window(S, [h[5]], reads(h[5], 3, 70)),
          Window(S, [h[6]], reads(h[6], 2) + [ReadRec("", [], ps.MQ, S + 5)])]
    ws += [Window(S, [ps.rnd(rng, 50)], reads(h[0], 2)) for _ in range(6)]
    return pack(ws)


def test_selection_eligibility_first_windows_determinism_and_offsets(lib):
    pb = sample_batch()
    p = capi.params_cli_defaults()
    cls = fc.faster_classes(p, pb, True)
    assert list(cls[:7]) == [0, 2, 0, 0, 2, 0, 1]
    ordinary = [0, 2, 5] + list(range(7, 13))
    for options, eligible, first in ((0, ordinary, {2, 5}), (ALL, sorted(ordinary + [1, 4]), {2, 5})):
        for seed in range(25):
            for want in (1, 2, 3, 4, 50):
                s = capi.AuditSample(p, pb, want, seed=seed, win_class=cls, faster=True, options=options)
                assert s.n_eligible == len(eligible) and set(s.chosen) <= set(eligible) and len(s.chosen) == min(want, len(eligible))
                n_first = len(first) + (1 if options else 0)
                if n_first <= want < len(eligible):
                    assert first <= set(s.chosen), (options, seed, want, s.chosen)      # the two shapes that size the launch's LDS
                    if options:
                        assert set(s.chosen) & {1, 4}, (seed, want, s.chosen)           # one long window
                t = capi.AuditSample(p, pb, want, seed=seed, win_class=cls, faster=True, options=options)
                assert np.array_equal(s.chosen, t.chosen) and np.array_equal(s.pair_off, t.pair_off)
    # a sample too small for the first windows is uniform; the seed matters beyond them
    assert len({tuple(capi.AuditSample(p, pb, 1, seed=s, win_class=cls, faster=True).chosen) for s in range(40)}) > 3
    assert len({tuple(capi.AuditSample(p, pb, 5, seed=s, win_class=cls, faster=True).chosen) for s in range(40)}) > 5
    assert {int(w) for s in range(40) for w in capi.AuditSample(p, pb, 3, seed=s, win_class=cls, faster=True, options=ALL).chosen} >= {1, 4}
    # without classes a window is classed by its shape
    s = capi.AuditSample(p, pb, 50, seed=1, faster=True)
    assert set(s.chosen) == set(ordinary)
    s = capi.AuditSample(p, pb, 50, seed=1, faster=True, options=ALL)
    assert set(s.chosen) == set(ordinary + [1, 4])
    # offsets and sizes against numpy
    a = pb.a
    for want, seed in ((0, 1), (4, 2), (9, 3), (1000, 5)):
        s = capi.AuditSample(p, pb, want, seed=seed, win_class=cls, faster=True, options=ALL)
        m = np.zeros(pb.n_windows, np.int64)
        m[s.chosen] = 1
        for got, full in ((s.pair_off, pb.win_pair_off), (s.hpos_off, pb.win_hpos_off), (s.varcov_off, pb.win_varcov_off)):
            assert np.array_equal(got, np.concatenate([[0], np.cumsum(np.diff(np.asarray(full, np.int64)) * m)]))
        assert (s.sizes.n_pairs, s.sizes.hpos_len, s.sizes.var_cov_len, s.sizes.n_windows) == (s.pair_off[-1], s.hpos_off[-1], s.varcov_off[-1], len(s.chosen))
        hl, rl = np.diff(a["hap_seq_off"]), np.diff(a["read_seq_off"])
        mh = max([hl[a["win_hap_off"][w]:a["win_hap_off"][w + 1]].max() for w in s.chosen], default=0)
        mr = max([rl[a["win_read_off"][w]:a["win_read_off"][w + 1]].max() for w in s.chosen], default=0)
        assert (s.sizes.max_hap_len, s.sizes.max_read_len) == (mh, mr)
        assert (s.audit_class[s.chosen] == capi.DD_WIN_LONG).all() and (np.delete(s.audit_class, s.chosen) == capi.DD_WIN_UNSUPPORTED).all()


# ---- headers and ABI ----
def test_headers_compile_as_c99_and_cxx_and_the_rule_is_the_tables(lib, tmp_path):
    """include/dindel_hmm.h and the rule of csrc/faster_shadow.h as C99 with -pedantic; the whole header (the model) as C++ host code."""
    src = tmp_path / "use_rule.c"
    src.write_text('#include <stdio.h>\n#include "dindel_tgi_amd/csrc/faster_shadow.h"\n'
                   'int main(void) {\n'
                   '  printf("%u %u %u %u %u %u\\n", au_compared_faster(DD_PAIR_OK, 1), au_compared_faster(DD_PAIR_OK, 0), au_compared_faster(DD_PAIR_NAN, 1),\n'
                   '         au_compared_faster(DD_PAIR_HAPSIZE, 0), au_compared_faster(DD_PAIR_LLPOS, 1), au_compared_faster(DD_PAIR_UNSUPPORTED, 1));\n'
                   '  return dd_audit_select_faster(NULL, NULL, NULL, 0, 0, 0, NULL, NULL, NULL, NULL, NULL) == DD_ERR_INVALID &&\n'
                   '         dd_audit_device_faster(NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL, 0, NULL) == DD_ERR_INVALID &&\n'
                   '         dd_audit_shadow_faster_host(NULL, NULL, NULL, NULL) == DD_ERR_INVALID &&\n'
                   '         dd_audit_compare_host_faster(NULL, NULL, NULL, NULL, NULL, 0) == DD_ERR_INVALID &&\n'
                   '         dd_audit_workspace_bytes_faster(NULL, NULL) == 0 ? 0 : 1;\n}\n')
    exe = tmp_path / "use_rule"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", ROOT, str(src), "-L", CSRC, "-ldindel_hmm",
                           "-Wl,-rpath," + CSRC, "-o", str(exe)])
    import torch
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = [int(v) for v in subprocess.check_output([str(exe)], env=env).decode().split()]
    every, cov = (1 << 18) - 1, (1 << 16) | (1 << 17)
    thrown = sum(1 << i for i in range(0, 13))
    assert out == [every, every & ~(1 << 17), thrown | cov, thrown | (1 << 16), 1, 1]
    cxx = tmp_path / "use_model.cpp"
    cxx.write_text('#include "dindel_tgi_amd/csrc/faster_shadow.h"\nint main() { return fs_status(5, 4, 36) == DD_PAIR_HAPSIZE && fs_bmid(1000u, 100, 2000u, 36) == 0 '
                   '&& fs_bmid(1000u, 100, 10u, 36) == 35 ? 0 : 1; }\n')
    subprocess.check_call([HIPCC, "-std=c++17", "-Wall", "-Werror", "-I", ROOT, str(cxx), "-o", str(tmp_path / "use_model")])
    subprocess.check_call([str(tmp_path / "use_model")], env=env)
    assert lib.dd_abi_version() == capi.ABI_VERSION == 13                      # new symbols only: the version is the parent's
    for name in ("dd_audit_select_faster", "dd_audit_workspace_bytes_faster", "dd_audit_device_faster", "dd_audit_last_launch_faster",
                 "dd_audit_shadow_faster_host", "dd_audit_compare_host_faster"):
        assert hasattr(lib, name) and name in capi.EXPORTS


def test_entries_validate_and_the_launch_has_no_cpu_fallback(lib):
    import torch
    from dindel_tgi_amd.batch import alloc_result
    pb = synth.generate(6, H=3, R=5, L=40, hap_len=100, seed=11)
    p = capi.params_cli_defaults()
    b = pb.ctypes_batch()
    W = pb.n_windows
    cls = np.zeros(W, np.uint8)
    off = [np.zeros(W + 1, np.int64) for _ in range(3)]
    sizes = capi.dd_audit_sizes()

    def select(params=p, batch=b, out=cls, sz=sizes, options=0):
        return lib.dd_audit_select_faster(C.byref(params) if params is not None else None, C.byref(batch) if batch is not None else None, None, options,
                                          1, 2, out.ctypes.data_as(capi.c_u8p) if out is not None else None,
                                          *[o.ctypes.data_as(capi.c_i64p) for o in off], C.byref(sz) if sz is not None else None)
    assert select(params=None) == capi.DD_ERR_INVALID and "params" in capi.last_error()
    assert select(batch=None) == capi.DD_ERR_INVALID
    assert select(out=None) == capi.DD_ERR_INVALID and "output" in capi.last_error()
    assert select(sz=None) == capi.DD_ERR_INVALID
    assert select(options=capi.DD_OPT_LONG_WINDOWS) == capi.DD_ERR_INVALID and "option" in capi.last_error()
    bad = capi.params_cli_defaults()
    bad.maxLengthDel = 32
    assert select(params=bad) == capi.DD_ERR_UNSUPPORTED
    assert select() == W and select(options=ALL) == W

    smp = capi.AuditSample(p, pb, W, faster=True)
    arrs, res = alloc_result(pb)
    sh = fc.poisoned_shadow(smp)
    shres = fc.result_struct(sh)
    v = smp.view()
    other = smp.view()
    other.n_windows = W + 1
    nullv = smp.view()
    nullv.pair_off = None

    def shadow(params=p, batch=b, view=v, out=shres):
        return lib.dd_audit_shadow_faster_host(C.byref(params) if params is not None else None, C.byref(batch) if batch is not None else None,
                                               C.byref(view) if view is not None else None, C.byref(out) if out is not None else None)
    assert shadow(params=None) == capi.DD_ERR_INVALID and shadow(batch=None) == capi.DD_ERR_INVALID and shadow(out=None) == capi.DD_ERR_INVALID
    assert shadow(view=None) == capi.DD_ERR_INVALID and "view" in capi.last_error()
    assert shadow(view=other) == capi.DD_ERR_INVALID and "windows" in capi.last_error()
    assert shadow(view=nullv) == capi.DD_ERR_INVALID and "null array" in capi.last_error()
    assert shadow(out=fc.result_struct(sh, null=("status",))) == capi.DD_ERR_INVALID and "status" in capi.last_error()
    assert shadow() == 0
    buf = capi.audit_report_buffer(4)

    def compare(batch=b, primary=res, view=v, out=shres, report=buf.ctypes.data, cap=4):
        return lib.dd_audit_compare_host_faster(C.byref(batch) if batch is not None else None, C.byref(primary) if primary is not None else None,
                                                C.byref(view) if view is not None else None, C.byref(out) if out is not None else None, report, cap)
    assert compare(batch=None) == capi.DD_ERR_INVALID and compare(primary=None) == capi.DD_ERR_INVALID and compare(out=None) == capi.DD_ERR_INVALID
    assert compare(report=None) == capi.DD_ERR_INVALID and compare(view=None) == capi.DD_ERR_INVALID and compare(view=other) == capi.DD_ERR_INVALID
    assert compare(cap=-1) == capi.DD_ERR_INVALID and "max_records" in capi.last_error()
    assert compare(out=fc.result_struct(sh, null=("ll",))) == capi.DD_ERR_INVALID and "ll and status" in capi.last_error()
    assert compare() == 0

    # the device-pointer entry: validation first, then the missing device
    db = capi.dd_device_batch()
    db.n_windows, db.n_haps, db.n_reads, db.n_qual = W, pb.n_haps, pb.n_reads, b.n_qual
    inputs = ("win_hap_off", "win_read_off", "read_seq_off", "win_pair_off", "win_hpos_off", "win_varcov_off", "win_hap_start", "hap_seq_off", "hap_seq",
              "read_seq", "read_qidx", "read_mqidx", "read_start", "tables", "hap_var_off", "hap_var")
    for k in inputs:
        setattr(db, k, 256)
    dres, dsh = capi.dd_device_result(), capi.dd_device_result()
    for k in ("ll", "status"):
        setattr(dres, k, 256)
        setattr(dsh, k, 256)
    assert lib.dd_audit_workspace_bytes_faster(C.byref(p), C.byref(v)) == 0 and lib.dd_audit_workspace_bytes_faster(C.byref(p), None) == 0
    lsmp = capi.AuditSample(ps.params_for(5, 0), fc.long_batch(), 4, faster=True, options=ALL)
    lv = lsmp.view()
    ws_bytes = lib.dd_audit_workspace_bytes_faster(C.byref(p), C.byref(lv))
    per_wave = 32 * 1025 + 16 * 65 + 16 * 129                            # tile over histogram, path, mapState: 16-byte pieces
    assert ws_bytes == -(-lsmp.sizes.n_pairs // 4) * 4 * per_wave, (ws_bytes, lsmp.sizes.n_pairs)

    def device(params=p, batch=db, primary=dres, view=v, out=dsh, report=256, cap=4, ws=None, wsb=0):
        return lib.dd_audit_device_faster(C.byref(params) if params is not None else None, C.byref(batch) if batch is not None else None,
                                          C.byref(primary) if primary is not None else None, C.byref(view) if view is not None else None,
                                          C.byref(out) if out is not None else None, report, cap, ws, wsb, None)
    assert device(params=None) == capi.DD_ERR_INVALID
    assert device(batch=None) == capi.DD_ERR_INVALID and device(primary=None) == capi.DD_ERR_INVALID and device(out=None) == capi.DD_ERR_INVALID
    assert device(report=None) == capi.DD_ERR_INVALID and device(report=260) == capi.DD_ERR_INVALID and "aligned" in capi.last_error()
    assert device(cap=-1) == capi.DD_ERR_INVALID
    assert device(view=None) == capi.DD_ERR_INVALID and device(view=other) == capi.DD_ERR_INVALID
    assert device(out=capi.dd_device_result()) == capi.DD_ERR_INVALID and "ll and status" in capi.last_error()
    nooff = capi.dd_device_batch()
    nooff.n_windows, nooff.n_haps, nooff.n_reads, nooff.n_qual = W, pb.n_haps, pb.n_reads, b.n_qual
    assert device(batch=nooff) == capi.DD_ERR_INVALID and "offset array" in capi.last_error()
    db.tables = None
    assert device() == capi.DD_ERR_INVALID and "input array" in capi.last_error()
    db.tables = 256
    otherq = smp.view()
    otherq.n_qual = b.n_qual + 1
    assert device(view=otherq) == capi.DD_ERR_INVALID and "quality" in capi.last_error()
    ldb = capi.dd_device_batch()
    ldb.n_windows, ldb.n_haps, ldb.n_reads, ldb.n_qual = lsmp.n_windows, 6, 16, lsmp.n_qual
    for k in inputs:
        setattr(ldb, k, 256)
    assert device(batch=ldb, view=lv, ws=256, wsb=ws_bytes - 1) == capi.DD_ERR_INVALID and "dd_audit_workspace_bytes_faster" in capi.last_error()
    assert device(batch=ldb, view=lv, ws=None, wsb=ws_bytes) == capi.DD_ERR_INVALID
    if not torch.cuda.is_available():
        assert device() == capi.DD_ERR_NO_DEVICE and "no CPU fallback" in capi.last_error()
        assert device(batch=ldb, view=lv, ws=256, wsb=ws_bytes) == capi.DD_ERR_NO_DEVICE
    assert capi.audit_last_launch_faster()["pairs"] == 0


# ---- independence ----
def test_new_sources_name_none_of_the_shared_faster_files():
    """The shadow shares no text with the two --faster kernels: the new sources include (or mention by file name) none of the model header,
    its two fragments and the long kernel's header, and define their own synchronisation and fold."""
    shared = ("faster_model.h", "faster_sstate.inc", "faster_pair_end.inc", "faster_long_kernel.h")
    for name in NEW_SOURCES:
        text = open(os.path.join(CSRC, name)).read()
        for s in shared:
            assert s not in text, "%s names %s" % (name, s)
        for inc in re.findall(r'#\s*include\s*"([^"]+)"', text):
            assert os.path.basename(inc) in ("dindel_hmm.h", "hmm_kernel.h", "kernel_common.h", "audit_kernel.h", "faster_shadow.h", "capi_internal.h"), (name, inc)
        assert "ddfm" not in text and "FOLD(" not in text and "wave_sync" not in text and "asm" not in text.replace("assembly", ""), name


def test_check_program_under_address_and_undefined_sanitizers(tmp_path):
    """tests/audit_faster_check.cpp with the library's host units that make no HIP call (faster_shadow_host.cpp, audit_host.cpp,
    batch_host.cpp, plan.cpp), host code only, under AddressSanitizer and UBSan; run directly."""
    exe = str(tmp_path / "audit_faster_check")
    subprocess.check_call([HIPCC, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", *"-Xarch_host -fsanitize=address,undefined".split(),
                           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "audit_faster_check.cpp")]
                          + [os.path.join(CSRC, u + ".cpp") for u in ("faster_shadow_host", "audit_host", "batch_host", "plan")])
    env = {k: v for k, v in os.environ.items() if not k.startswith("DD_")}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.endswith("audit_faster_check: ok\n") and r.stderr == "", (r.stdout[-2000:], r.stderr[-4000:])
