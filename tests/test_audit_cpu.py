"""CPU-side checks of the audit (dd_audit_select, dd_audit_compare_host, dd_audit_device, dd_compute_likelihoods_audit): declarations,
validation, no CPU fallback for the launches, the sample's rules, the comparison rule of csrc/audit_kernel.h on oracle results with planted
differences against a numpy restatement written unlike it, and selection plus comparison over random batches in a stand-alone program
under AddressSanitizer and UBSan.  No compute on a device here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from dindel_tgi_amd import capi, synth
from tests import _audit_cases as ac
from tests import _path_scenarios as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dindel_tgi_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_headers_compile_as_c99_and_the_constants_agree(lib, tmp_path):
    """include/dindel_hmm.h and the rule the kernel and the CPU evaluation share (csrc/audit_kernel.h), as C99 with -pedantic."""
    src = tmp_path / "use_audit.c"
    src.write_text('#include <stdio.h>\n#include "dindel_tgi_amd/csrc/audit_kernel.h"\n'
                   'int main(void) {\n'
                   '  printf("%d %d %d %d %d ", DD_AUDIT_N_FIELDS, DD_AUDIT_FIELD_status, DD_AUDIT_FIELD_ll, DD_AUDIT_FIELD_hpos, DD_AUDIT_FIELD_var_fcov);\n'
                   '  printf("%d %d %d ", (int)sizeof(dd_audit_record), (int)sizeof(dd_audit_report), (int)DD_AUDIT_REPORT_BYTES(3));\n'
                   '  printf("%u %u %u %u ", au_compared(DD_PAIR_OK, 1), au_compared(DD_PAIR_LLPOS, 0), au_compared(DD_PAIR_HAPSIZE, 1), au_compared(DD_PAIR_UNSUPPORTED, 1));\n'
                   '  printf("%d %d %d %d\\n", au_field_size(DD_AUDIT_FIELD_status), au_field_size(DD_AUDIT_FIELD_mLogBQ), au_field_size(DD_AUDIT_FIELD_offHapHMQ), au_field_size(DD_AUDIT_FIELD_hpos));\n'
                   '  return dd_audit_select(NULL, NULL, NULL, 0, 0, NULL, NULL, NULL, NULL, NULL) == DD_ERR_INVALID &&\n'
                   '         dd_audit_device(NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL, 0, NULL) == DD_ERR_INVALID &&\n'
                   '         dd_audit_compare_host(NULL, NULL, NULL, NULL, NULL, 0) == DD_ERR_INVALID &&\n'
                   '         dd_compute_likelihoods_audit(NULL, NULL, NULL, 0, 0, 0, 0, NULL, 0) == DD_ERR_INVALID &&\n'
                   '         dd_audit_workspace_bytes(NULL, NULL) == 0 ? 0 : 1;\n}\n')
    exe = tmp_path / "use_audit"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", ROOT, str(src),
                           "-L", CSRC, "-ldindel_hmm", "-Wl,-rpath," + CSRC, "-o", str(exe)])
    import torch
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = [int(v) for v in subprocess.check_output([str(exe)], env=env).decode().split()]
    every = (1 << 18) - 1
    cov = (1 << 16) | (1 << 17)
    assert out == [18, 0, 1, 15, 17, 40, C.sizeof(capi.dd_audit_report), C.sizeof(capi.dd_audit_report) + 120,
                   every, every & ~(1 << 17), 1 | 2 | cov, 1, 4, 8, 1, 2]
    assert C.sizeof(capi.dd_audit_report) == 8 * (2 + 2 * 18) and C.sizeof(capi.dd_audit_record) == 40
    assert capi.AUDIT_FIELDS[0] == "status" and capi.AUDIT_FIELDS[15:] == ["hpos", "var_covered", "var_fcov"]
    assert set(capi.AUDIT_FIELDS) == {k for k, _t in capi.RESULT_FIELDS} - {"onHap"}
    assert lib.dd_abi_version() == capi.ABI_VERSION == 13                      # new symbols only: the version is the parent's
    for name in ("dd_audit_select", "dd_audit_workspace_bytes", "dd_audit_device", "dd_audit_last_launch", "dd_audit_compare_host",
                 "dd_compute_likelihoods_audit"):
        assert hasattr(lib, name) and name in capi.EXPORTS


def small_batch():
    return synth.generate(6, H=3, R=5, L=40, hap_len=100, seed=11)


def test_entries_validate_and_the_launches_have_no_cpu_fallback(lib):
    import torch
    from dindel_tgi_amd.batch import alloc_result
    pb = small_batch()
    p = capi.params_cli_defaults()
    b = pb.ctypes_batch()
    W = pb.n_windows
    cls = np.zeros(W, np.uint8)
    off = [np.zeros(W + 1, np.int64) for _ in range(3)]
    sizes = capi.dd_audit_sizes()

    def select(params=p, batch=b, out=cls, sz=sizes):
        return lib.dd_audit_select(C.byref(params) if params is not None else None, C.byref(batch) if batch is not None else None, None, 1, 2,
                                   out.ctypes.data_as(capi.c_u8p) if out is not None else None, *[o.ctypes.data_as(capi.c_i64p) for o in off],
                                   C.byref(sz) if sz is not None else None)
    assert select(params=None) == capi.DD_ERR_INVALID and "params" in capi.last_error()
    assert select(batch=None) == capi.DD_ERR_INVALID
    assert select(out=None) == capi.DD_ERR_INVALID and "output" in capi.last_error()
    assert select(sz=None) == capi.DD_ERR_INVALID
    bad = capi.params_cli_defaults()
    bad.maxLengthDel = 32
    assert select(params=bad) == capi.DD_ERR_UNSUPPORTED
    assert select() == W

    # the CPU evaluation
    smp = capi.AuditSample(p, pb, W)
    arrs, res = alloc_result(pb)
    sh = ac.shadow_from(pb, smp, arrs)
    shres = ac.result_struct(sh)
    buf = capi.audit_report_buffer(4)
    v = smp.view()

    def compare(batch=b, primary=res, view=v, shadow=shres, report=buf.ctypes.data, cap=4):
        return lib.dd_audit_compare_host(C.byref(batch) if batch is not None else None, C.byref(primary) if primary is not None else None,
                                         C.byref(view) if view is not None else None, C.byref(shadow) if shadow is not None else None, report, cap)
    assert compare(batch=None) == capi.DD_ERR_INVALID
    assert compare(primary=None) == capi.DD_ERR_INVALID and compare(shadow=None) == capi.DD_ERR_INVALID and compare(report=None) == capi.DD_ERR_INVALID
    assert compare(view=None) == capi.DD_ERR_INVALID and "view" in capi.last_error()
    assert compare(cap=-1) == capi.DD_ERR_INVALID and "max_records" in capi.last_error()
    other = smp.view()
    other.n_windows = W + 1
    assert compare(view=other) == capi.DD_ERR_INVALID and "windows" in capi.last_error()
    nullv = smp.view()
    nullv.pair_off = None
    assert compare(view=nullv) == capi.DD_ERR_INVALID and "null array" in capi.last_error()
    assert compare(shadow=ac.result_struct(sh, null=("status",))) == capi.DD_ERR_INVALID and "status" in capi.last_error()
    assert compare() == 0

    # the device-pointer entry: validation first, then the missing device
    db = capi.dd_device_batch()
    db.n_windows, db.n_haps, db.n_reads, db.n_qual = W, pb.n_haps, pb.n_reads, b.n_qual
    for k in ("win_hap_off", "win_read_off", "read_seq_off", "win_pair_off", "win_hpos_off", "win_varcov_off"):
        setattr(db, k, 256)
    dres, dsh = capi.dd_device_result(), capi.dd_device_result()
    for k in ("ll", "status"):
        setattr(dres, k, 256)
        setattr(dsh, k, 256)
    ws_bytes = lib.dd_audit_workspace_bytes(C.byref(p), C.byref(v))
    assert ws_bytes > 0 and lib.dd_audit_workspace_bytes(C.byref(p), None) == 0

    def device(params=p, batch=db, primary=dres, view=v, shadow=dsh, report=256, cap=4, ws=256, wsb=ws_bytes):
        return lib.dd_audit_device(C.byref(params) if params is not None else None, C.byref(batch) if batch is not None else None,
                                   C.byref(primary) if primary is not None else None, C.byref(view) if view is not None else None,
                                   C.byref(shadow) if shadow is not None else None, report, cap, ws, wsb, None)
    assert device(params=None) == capi.DD_ERR_INVALID
    assert device(batch=None) == capi.DD_ERR_INVALID and device(primary=None) == capi.DD_ERR_INVALID and device(shadow=None) == capi.DD_ERR_INVALID
    assert device(report=None) == capi.DD_ERR_INVALID and device(report=260) == capi.DD_ERR_INVALID and "aligned" in capi.last_error()
    assert device(cap=-1) == capi.DD_ERR_INVALID
    assert device(view=None) == capi.DD_ERR_INVALID and device(view=other) == capi.DD_ERR_INVALID
    assert device(shadow=capi.dd_device_result()) == capi.DD_ERR_INVALID and "ll and status" in capi.last_error()
    assert device(ws=None) == capi.DD_ERR_INVALID and device(wsb=ws_bytes - 1) == capi.DD_ERR_INVALID and "dd_audit_workspace_bytes" in capi.last_error()
    nooff = capi.dd_device_batch()
    nooff.n_windows, nooff.n_haps, nooff.n_reads, nooff.n_qual = W, pb.n_haps, pb.n_reads, b.n_qual
    assert device(batch=nooff) == capi.DD_ERR_INVALID and "offset array" in capi.last_error()
    otherq = smp.view()
    otherq.n_qual = b.n_qual + 1
    assert device(view=otherq) == capi.DD_ERR_INVALID and "quality" in capi.last_error()

    # the host-pointer entry
    def host(options=0, report=buf.ctypes.data, cap=4, result=res, want=2):
        return lib.dd_compute_likelihoods_audit(C.byref(p), C.byref(b), C.byref(result), 0, options, 5, want, report, cap)
    for opt in (capi.DD_OPT_LONG_WINDOWS_FASTER, 4):
        assert host(options=opt) == capi.DD_ERR_INVALID and "option" in capi.last_error()
    assert host(report=None) == capi.DD_ERR_INVALID and "report" in capi.last_error()
    assert host(cap=-1) == capi.DD_ERR_INVALID
    assert host(result=capi.dd_result()) == capi.DD_ERR_INVALID and "ll and status" in capi.last_error()
    if not torch.cuda.is_available():
        assert device() == capi.DD_ERR_NO_DEVICE and "no CPU fallback" in capi.last_error()
        for kw in (dict(), dict(options=capi.DD_OPT_LONG_WINDOWS), dict(want=0)):
            assert host(**kw) == capi.DD_ERR_NO_DEVICE and "no CPU fallback" in capi.last_error()
    # a batch without pairs is finished before the device is asked for, with an empty report
    from tests import _cigar_cases as cc
    empty = cc.csr_batch([([], [20, 20]), ([30], [])])
    e_arrs, e_res = alloc_result(empty)
    eb = empty.ctypes_batch()
    buf[...] = 0xFF
    assert lib.dd_compute_likelihoods_audit(C.byref(p), C.byref(eb), C.byref(e_res), 0, 0, 5, 2, buf.ctypes.data, 4) == 0
    rep = capi.audit_report(buf, 4)
    assert rep["n_pairs"] == 0 and rep["n_diff"] == 0 and not any(rep["compared"].values())


def test_selection_is_a_function_of_seed_and_batch(lib):
    pb = synth.generate(40, H=3, R=5, L=40, hap_len=100, seed=11)
    p = capi.params_cli_defaults()
    a, b = capi.AuditSample(p, pb, 7, seed=123), capi.AuditSample(p, pb, 7, seed=123)
    assert np.array_equal(a.chosen, b.chosen) and len(a.chosen) == 7 and a.n_eligible == 40
    for k in ("pair_off", "hpos_off", "varcov_off"):
        assert np.array_equal(getattr(a, k), getattr(b, k))
    # after other calls in between (no call history), and from another thread
    capi.AuditSample(p, pb, 3, seed=9)
    import threading
    got = []
    t = threading.Thread(target=lambda: got.append(capi.AuditSample(p, pb, 7, seed=123).chosen))
    t.start()
    t.join()
    assert np.array_equal(got[0], a.chosen)
    samples = [tuple(capi.AuditSample(p, pb, 7, seed=s).chosen) for s in range(20)]
    assert len(set(samples)) > 10                                      # the seed matters
    # uniform over the eligible windows: every window is chosen by some seed, none by nearly all
    counts = np.zeros(40, int)
    for s in range(400):
        counts[capi.AuditSample(p, pb, 4, seed=s).chosen] += 1
    assert counts.min() >= 10 and counts.max() <= 90, counts            # expected 40 each (binomial, sd 6)
    # another batch, same seed: its own choice
    other = synth.generate(40, H=3, R=5, L=40, hap_len=100, seed=12)
    assert len(capi.AuditSample(p, other, 7, seed=123).chosen) == 7


def edge_batch():
    """Windows 0, 3: ordinary; 1: haplotypes without reads; 2: reads without haplotypes; 4: a 900-bp haplotype (long with the option, else
    unsupported); 5: ordinary; 6: an empty read (unsupported)."""
    from dindel_tgi_amd.batch import Window, ReadRec, pack
    rng = np.random.default_rng(5)
    S = ps.HAP_START
    h = [ps.rnd(rng, n) for n in (60, 60, 60, 70, 900, 80, 60)]
    reads = lambda hap, n: ps.spread_reads(rng, hap, n, 30)
    ws = [Window(S, [h[0], h[0][:30] + h[0][31:]], reads(h[0], 4)),
          Window(S, [h[1]], []),
          Window(S, [], reads(h[2], 3)),
          Window(S, [h[3]], reads(h[3], 5)),
          Window(S, [h[4]], reads(h[4], 2)),
          Window(S, [h[5], h[5][:40] + "AC" + h[5][40:]], reads(h[5], 3)),
          Window(S, [h[6]], reads(h[6], 2) + [ReadRec("", [], ps.MQ, S + 5)])]
    return pack(ws)


@pytest.mark.parametrize("long_windows", [False, True])
def test_only_ordinary_windows_with_pairs_are_eligible(lib, long_windows):
    pb = edge_batch()
    p = capi.params_cli_defaults()
    if long_windows:
        cls, _mx, _n = capi.screen_windows_ex(p, pb, capi.DD_OPT_LONG_WINDOWS)
        assert cls[4] == capi.DD_WIN_LONG and cls[6] == capi.DD_WIN_UNSUPPORTED
    else:
        cls = ac.main_classes(lib, p, pb)
        assert cls[4] != 0 and cls[6] != 0
    for seed in range(30):
        for want in (1, 2, 3, 50):
            s = capi.AuditSample(p, pb, want, seed=seed, win_class=cls)
            assert s.n_eligible == 3 and set(s.chosen) <= {0, 3, 5} and len(s.chosen) == min(want, 3), (seed, want, s.chosen)
            assert (s.audit_class[s.chosen] == capi.DD_WIN_LONG).all() and (np.delete(s.audit_class, s.chosen) == capi.DD_WIN_UNSUPPORTED).all()
    # without classes every window counts as ordinary, but one the long-window kernel cannot take is still left out
    s = capi.AuditSample(p, pb, 50, seed=1)
    assert set(s.chosen) == {0, 3, 4, 5}


def test_every_launch_class_of_a_ragged_batch_is_in_the_sample(lib):
    pb = synth.generate_ragged(48, seed=0x5EED4, max_reads=40)
    p = capi.params_cli_defaults()
    b = pb.ctypes_batch()
    cls = capi.dd_length_classes()
    lst = np.zeros(pb.n_haps * capi.N_READ_CLASSES + 1, np.int32)
    assert lib.dd_build_length_classes(C.byref(b), None, C.byref(p), lst.ctypes.data_as(capi.c_i32p), C.byref(cls)) == 0
    hap_window = np.repeat(np.arange(pb.n_windows), np.diff(pb.a["win_hap_off"]))
    class_windows = [set(hap_window[lst[cls.launch[i].list_off:cls.launch[i].list_off + cls.launch[i].list_len]]) for i in range(cls.n_launches)]
    n_cls = len(class_windows)
    assert n_cls >= 3, n_cls                                             # the batch is ragged enough to mean something
    for seed in range(25):
        for want in (n_cls, n_cls + 2, 20):
            s = capi.AuditSample(p, pb, want, seed=seed)
            assert len(s.chosen) == want
            assert all(ws & set(s.chosen) for ws in class_windows), (seed, want, s.chosen)
    # a sample too small to hold every class is uniform: no class is preferred
    assert len(capi.AuditSample(p, pb, n_cls - 1, seed=3).chosen) == n_cls - 1
    # some class is rare enough that a uniform choice of n_cls windows would often miss it
    assert min(len(ws) for ws in class_windows) <= pb.n_windows // 4


def test_offsets_and_sizes_are_prefix_sums_over_the_chosen_windows(lib):
    pb = synth.generate_ragged(30, seed=77, max_reads=30)
    p = capi.params_cli_defaults()
    a = pb.a
    for want, seed in ((0, 1), (1, 2), (9, 3), (30, 4), (1000, 5)):
        s = capi.AuditSample(p, pb, want, seed=seed)
        n = min(max(want, 0), pb.n_windows)
        assert len(s.chosen) == n == s.sizes.n_windows and s.n_eligible == pb.n_windows
        m = np.zeros(pb.n_windows, np.int64)
        m[s.chosen] = 1
        for got, full in ((s.pair_off, pb.win_pair_off), (s.hpos_off, pb.win_hpos_off), (s.varcov_off, pb.win_varcov_off)):
            want_off = np.concatenate([[0], np.cumsum(np.diff(np.asarray(full, np.int64)) * m)])
            assert np.array_equal(got, want_off)
        assert (s.sizes.n_pairs, s.sizes.hpos_len, s.sizes.var_cov_len) == (s.pair_off[-1], s.hpos_off[-1], s.varcov_off[-1])
        hl, rl = np.diff(a["hap_seq_off"]), np.diff(a["read_seq_off"])
        mh = max([hl[a["win_hap_off"][w]:a["win_hap_off"][w + 1]].max() for w in s.chosen], default=0)
        mr = max([rl[a["win_read_off"][w]:a["win_read_off"][w + 1]].max() for w in s.chosen], default=0)
        assert (s.sizes.max_hap_len, s.sizes.max_read_len) == (mh, mr)
        if n == pb.n_windows:
            assert np.array_equal(s.pair_off, pb.win_pair_off)
    assert len(capi.AuditSample(p, pb, -3).chosen) == 0


# ---- the comparison ----
def compare_case(null=()):
    pb, index, p, want = ac.scenario()
    cls = ac.main_classes(capi.load(), p, pb)
    smp = capi.AuditSample(p, pb, pb.n_windows, win_class=cls)
    primary = {k: np.array(v, copy=True) for k, v in want.items()}
    shadow = ac.shadow_from(pb, smp, want)
    return pb, index, p, want, smp, primary, shadow


def run_compare(pb, primary, smp, shadow, cap=64, null_p=(), null_s=()):
    return capi.audit_compare_host(pb, ac.result_struct(primary, null_p), smp, ac.result_struct(shadow, null_s), cap)


def test_a_copy_of_the_oracle_results_gives_no_difference_and_exact_counts():
    pb, index, p, want, smp, primary, shadow = compare_case()
    rep = run_compare(pb, primary, smp, shadow)
    assert rep["n_diff"] == 0 and not any(rep["diff"].values()) and rep["records"] == []
    assert rep["n_pairs"] == smp.sizes.n_pairs
    has_flank = pb.hap_var_flank is not None and len(pb.hap_var_flank) > 0
    assert has_flank
    assert rep["compared"] == ac.expected_compared(pb, want["status"], smp.chosen, has_flank)
    st = want["status"][:pb.n_pairs]
    assert (st == capi.DD_PAIR_HAPSIZE).any() and len(smp.chosen) < pb.n_windows        # the scenario has both kinds of pair, and a screened window


def shadow_index(pb, smp, k, e):
    """Where element e of the primary's array k lies in the shadow."""
    full = {"hpos": pb.win_hpos_off, "var_covered": pb.win_varcov_off, "var_fcov": pb.win_varcov_off}.get(k, pb.win_pair_off)
    mine = {"hpos": smp.hpos_off, "var_covered": smp.varcov_off, "var_fcov": smp.varcov_off}.get(k, smp.pair_off)
    w = int(np.searchsorted(np.asarray(full), e, side="right")) - 1
    assert w in smp.chosen
    return int(mine[w]) + e - int(full[w]), w


def test_one_inverted_bit_in_each_field_is_reported_with_both_values():
    pb, index, p, want, smp, primary, shadow = compare_case()
    elem = ps.element_pairs(pb)
    st = want["status"][:pb.n_pairs]
    in_sample = np.isin(ac.window_of_pairs(pb), smp.chosen)
    ok = np.nonzero(in_sample & (st == capi.DD_PAIR_OK))[0]
    pair = int(ok[len(ok) // 2])
    hp = np.nonzero(elem["hpos"][:pb.hpos_len] == pair)[0]
    vc = np.nonzero(np.isin(elem["var_covered"][:pb.var_cov_len], ok))[0]
    targets = [(k, pair) for k in capi.AUDIT_FIELDS[:15]] + [("hpos", int(hp[0])), ("hpos", int(hp[-1])), ("var_covered", int(vc[0])), ("var_fcov", int(vc[-1]))]
    for side in ("primary", "shadow"):
        for k, e in targets:
            arrs = primary if side == "primary" else shadow
            at, w = (e, None) if side == "primary" else shadow_index(pb, smp, k, e)
            if side == "primary":
                w = shadow_index(pb, smp, k, e)[1]
            raw = arrs[k].view(np.uint8).reshape(len(arrs[k]), -1)
            raw[at, 0] ^= 0x04
            try:
                rep = run_compare(pb, primary, smp, shadow)
            finally:
                raw[at, 0] ^= 0x04
            assert rep["n_diff"] == 1 and rep["diff"][k] == 1 and sum(rep["diff"].values()) == 1, (side, k, rep["diff"])
            r = rep["records"][0]
            owner = int(elem[k][e]) if k in ac.PER_ELEMENT else e
            bits = int(np.asarray(want[k][e:e + 1]).view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[want[k].dtype.itemsize])[0])
            flipped = bits ^ 0x04
            assert (r["window"], r["field"], r["pair"], r["index"]) == (w, k, owner, e), (side, k, r)
            assert (r["primary_bits"], r["shadow_bits"]) == ((flipped, bits) if side == "primary" else (bits, flipped)), (side, k, r)


def test_a_status_difference_hides_the_pairs_other_differences():
    pb, index, p, want, smp, primary, shadow = compare_case()
    st = want["status"][:pb.n_pairs]
    in_sample = np.isin(ac.window_of_pairs(pb), smp.chosen)
    pair = int(np.nonzero(in_sample & (st == capi.DD_PAIR_OK))[0][3])
    elem = ps.element_pairs(pb)
    primary["status"][pair] = capi.DD_PAIR_NAN
    primary["ll"][pair] += 1.0
    primary["numIndels"][pair] += 1
    primary["hpos"][np.nonzero(elem["hpos"][:pb.hpos_len] == pair)[0]] ^= 1
    rep = run_compare(pb, primary, smp, shadow)
    assert rep["n_diff"] == 1 and rep["diff"]["status"] == 1 and rep["records"][0]["field"] == "status" and rep["records"][0]["pair"] == pair
    assert (rep["records"][0]["primary_bits"], rep["records"][0]["shadow_bits"]) == (capi.DD_PAIR_NAN, capi.DD_PAIR_OK)
    base = ac.expected_compared(pb, want["status"], smp.chosen, True)
    L = int((elem["hpos"][:pb.hpos_len] == pair).sum())
    nv = int((elem["var_covered"][:pb.var_cov_len] == pair).sum())
    assert rep["compared"]["ll"] == base["ll"] - 1 and rep["compared"]["hpos"] == base["hpos"] - L and rep["compared"]["var_covered"] == base["var_covered"] - nv
    assert rep["compared"]["status"] == base["status"]


def test_unowned_elements_outside_windows_and_null_fields_are_not_compared():
    pb, index, p, want, smp, primary, shadow = compare_case()
    st = want["status"][:pb.n_pairs]
    elem = ps.element_pairs(pb)
    in_sample = np.isin(ac.window_of_pairs(pb), smp.chosen)
    hs = np.nonzero(in_sample & (st == capi.DD_PAIR_HAPSIZE))[0]
    assert hs.size
    # a hapSize-error pair: everything but status, ll and the coverage flags is garbage on both sides, and different garbage
    for k in capi.AUDIT_FIELDS[2:15]:
        primary[k][hs] = primary[k][hs] + 3
    primary["hpos"][np.isin(elem["hpos"][:pb.hpos_len], hs)] = 0x5A5A
    # a window outside the sample (the screened one): all of it differs
    out = np.nonzero(~in_sample)[0]
    assert out.size
    primary["ll"][out] = 1.0
    primary["status"][out] = 7
    # onHap is never compared
    primary["onHap"][...] ^= 1
    rep = run_compare(pb, primary, smp, shadow)
    assert rep["n_diff"] == 0, rep["records"][:3]
    # ... while an owned element of a hapSize-error pair is
    primary["ll"][hs[0]] = -1.0
    rep = run_compare(pb, primary, smp, shadow)
    assert rep["n_diff"] == 1 and rep["records"][0]["field"] == "ll" and rep["records"][0]["pair"] == int(hs[0])
    primary["ll"][hs[0]] = want["ll"][hs[0]]
    # NULL fields on either side are skipped, with their differences
    ok = int(np.nonzero(in_sample & (st == capi.DD_PAIR_OK))[0][0])
    primary["llOn"][ok] += 1.0
    primary["var_fcov"][...] ^= 1
    assert run_compare(pb, primary, smp, shadow)["n_diff"] > 1
    for kw in (dict(null_p=("llOn", "var_fcov")), dict(null_s=("llOn", "var_fcov")), dict(null_p=("llOn",), null_s=("var_fcov",))):
        rep = run_compare(pb, primary, smp, shadow, **kw)
        assert rep["n_diff"] == 0 and rep["compared"]["llOn"] == 0 and rep["compared"]["var_fcov"] == 0 and rep["compared"]["llOff"] > 0, kw
    # a sample of some windows only: a difference in another window is not seen
    part = capi.AuditSample(p, pb, 2, seed=4, win_class=ac.main_classes(capi.load(), p, pb))
    outside = np.nonzero(~np.isin(ac.window_of_pairs(pb), part.chosen))[0]
    primary = {k: np.array(v, copy=True) for k, v in want.items()}
    primary["ll"][outside] = 2.0
    rep = run_compare(pb, primary, part, ac.shadow_from(pb, part, want))
    assert rep["n_diff"] == 0 and rep["n_pairs"] == part.sizes.n_pairs < pb.n_pairs


@pytest.mark.parametrize("cap", [0, 1, 2])
def test_a_small_record_cap_keeps_the_counts_right(cap):
    pb, index, p, want, smp, primary, shadow = compare_case()
    st = want["status"][:pb.n_pairs]
    in_sample = np.isin(ac.window_of_pairs(pb), smp.chosen)
    ok = np.nonzero(in_sample & (st == capi.DD_PAIR_OK))[0][:5]
    primary["ll"][ok] += 1.0
    primary["lastBase"][ok[:2]] += 1
    guard = capi.audit_report_buffer(cap + 1)
    guard[...] = 0xEE
    b = pb.ctypes_batch()
    v = smp.view()
    rc = capi.load().dd_audit_compare_host(C.byref(b), C.byref(ac.result_struct(primary)), C.byref(v), C.byref(ac.result_struct(shadow)), guard.ctypes.data, cap)
    assert rc == 0
    rep = capi.audit_report(guard, cap)
    assert rep["n_diff"] == 7 and rep["diff"]["ll"] == 5 and rep["diff"]["lastBase"] == 2 and len(rep["records"]) == cap
    assert (guard[C.sizeof(capi.dd_audit_report) + cap * C.sizeof(capi.dd_audit_record):] == 0xEE).all()          # nothing behind the last record it has room for


def test_check_program_under_address_and_undefined_sanitizers(tmp_path):
    """tests/audit_check.cpp with the library's host units that make no HIP call (audit_host.cpp, batch_host.cpp, plan.cpp), host code only,
    under AddressSanitizer and UBSan; run directly."""
    exe = str(tmp_path / "audit_check")
    subprocess.check_call([HIPCC, "-std=c++17", "-O1", "-g", "-Wall", *"-Xarch_host -fsanitize=address,undefined".split(), "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "audit_check.cpp")] + [os.path.join(CSRC, u + ".cpp") for u in ("audit_host", "batch_host", "plan")])
    env = {k: v for k, v in os.environ.items() if not k.startswith("DD_")}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.endswith("audit_check: ok\n") and r.stderr == "", (r.stdout[-2000:], r.stderr[-4000:])
