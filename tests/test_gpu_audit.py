"""The audit on the device: a sample of a launch's ordinary windows recomputed by dd_long_kernel into shadow buffers and compared, bit for bit,
with what the main kernels left in HBM (dd_audit_device, DeviceBatch(audit=N), dd_compute_likelihoods_audit).

  clean      every eligible window of a scenario batch (tests/_path_scenarios.py: every per-pair path, mapUnmappedReads on): no difference, the
             shadow bit-equal to the oracle on every element the rule names, and the number of elements compared per field equal to the
             number the oracle's statuses and the rule give
  builds     one window per haplotype-length class bound and the launch-shape recipes that select the other builds, at maxLengthDel 5, 10,
             11 and 20: no difference on any build the launch selects
  planted    bits inverted through torch in ll, hpos, var_fcov and status of audited pairs and in ll of a pair outside the sample: the report
             names exactly the planted ones
  guards     256-byte guards around primary, shadow and report, different poison in primary and shadow: nothing but the shadow's owned
             elements and the report is written, and the primary is byte-identical before and after and to a run without audit
  variants   more audited pairs than resident workgroups; a stream of its own with a second launch into the same buffers; long windows
             beside the audit; the host-pointer entry over two window blocks, with the test hook that plants a difference"""
import ctypes as C

import numpy as np
import pytest

from dindel_tgi_amd import capi, synth
from dindel_tgi_amd.batch import RESULT_DTYPES
from tests import _audit_cases as ac
from tests import _launch_shapes as ls
from tests import _path_scenarios as ps
from tests._output_ownership import GUARD, GUARD_BYTE, GuardedDevice

pytestmark = pytest.mark.gpu
SHADOW_POISON = 0x3C


@pytest.fixture(scope="module")
def lib():
    return capi.load()


def audited(dev):
    """launch(), launch_audit() -> the report (with shadow and sample)."""
    import torch
    dev.launch()
    dev.launch_audit()
    torch.cuda.synchronize()
    return dev.audit_results()


def owned_shadow(pb, smp, want):
    """-> ({field: expected shadow}, {field: mask of the shadow's elements the rule names}) from the oracle's arrays."""
    st_full = np.asarray(want["status"][:pb.n_pairs])
    exp = {k: np.array(v, copy=True) for k, v in want.items()}
    hapsize = st_full == capi.DD_PAIR_HAPSIZE
    exp["ll"][:pb.n_pairs][hapsize] = 0.0                      # what the library defines for a pair the reference throws for
    elem = ps.element_pairs(pb)
    for k in ("var_covered", "var_fcov"):
        exp[k][:pb.var_cov_len][hapsize[elem[k][:pb.var_cov_len]]] = 0
    sh = ac.shadow_from(pb, smp, exp)
    st = sh["status"][:smp.sizes.n_pairs]
    computed = np.isin(st, ac.COMPUTED)
    cov = computed | (st == capi.DD_PAIR_HAPSIZE)
    pair_of = ac.shadow_from(pb, smp, {k: (elem[k] if k in ac.PER_ELEMENT else np.arange(pb.n_pairs)) for k, _t in capi.RESULT_FIELDS if k != "onHap"})
    # a shadow element's pair, as an index into the shadow: its primary pair moved by its window's shift
    shift = np.zeros(pb.n_pairs, np.int64)
    for w in smp.chosen:
        shift[int(pb.win_pair_off[w]):int(pb.win_pair_off[w + 1])] = int(smp.pair_off[w]) - int(pb.win_pair_off[w])
    mask = {}
    for k in sh:
        n = {"hpos": smp.sizes.hpos_len, "var_covered": smp.sizes.var_cov_len, "var_fcov": smp.sizes.var_cov_len}.get(k, smp.sizes.n_pairs)
        own = pair_of[k][:n] + shift[pair_of[k][:n]]
        mask[k] = (np.ones(n, bool) if k == "status" else cov[own] if k in ("ll", "var_covered", "var_fcov") else computed[own])
        sh[k] = sh[k][:n]
    return sh, mask


def test_clean_audit_of_every_eligible_window(lib):
    from dindel_tgi_amd.device import DeviceBatch
    pb, index, p, want = ac.scenario()
    assert p.mapUnmappedReads == 1
    dev = DeviceBatch(pb, p, "cuda:0", audit=pb.n_windows, audit_seed=1)
    smp = dev.audit
    eligible = np.nonzero((ac.main_classes(lib, p, pb) == 0) & (np.diff(pb.win_pair_off) > 0))[0]
    assert list(smp.chosen) == list(eligible) and 0 < len(smp.chosen) < pb.n_windows
    rep = audited(dev)
    assert rep["n_diff"] == 0 and not any(rep["diff"].values()), rep["records"][:5]
    assert rep["n_pairs"] == smp.sizes.n_pairs
    # the audit itself: the shadow is the oracle's, on every element the rule names
    exp, mask = owned_shadow(pb, smp, want)
    for k, m in mask.items():
        got = rep["shadow"][k]
        bad = np.nonzero(m & (got.view(np.uint8).reshape(len(got), -1) != exp[k].view(np.uint8).reshape(len(got), -1)).any(axis=1))[0]
        assert bad.size == 0, "shadow %s[%d] is %r, the oracle has %r" % (k, int(bad[0]), got[bad[0]], exp[k][bad[0]])
    # an exact count of what was compared, from the oracle's statuses and the rule
    assert rep["compared"] == ac.expected_compared(pb, want["status"], smp.chosen, True)
    assert (np.asarray(want["status"])[:pb.n_pairs] == capi.DD_PAIR_HAPSIZE).any()
    log = capi.audit_last_launch()
    assert log["pairs"] == smp.sizes.n_pairs and log["K"] == 1 and log["max_hap"] == smp.sizes.max_hap_len and log["compare_grid"] > 0, log


BUILD_RECIPES = ("fold_hap61", "fold_hap62", "fold_hap125", "fold_hap126", "half_hap30", "half_hap94", "half_hap158", "lds_hap120_read100",
                 "scratch_hap120_read120", "two_waves_k3_read400")


@pytest.mark.parametrize("mld", [5, 10, 11, 20])
def test_no_difference_on_any_selectable_build(lib, mld):
    from dindel_tgi_amd.device import DeviceBatch
    p = ps.params_for(mld, 0)
    cases = {c["name"]: c for c in ls.load_cases()}
    batches = [("class bounds", synth.concat([synth.generate(1, H=1, R=6, L=36, hap_len=hl, seed=1000 + hl) for hl in ps.hap_lengths(mld)]))]
    batches += [(name, ls.build_batch(cases[name]["recipe"])[0]) for name in BUILD_RECIPES]
    builds, shapes = set(), set()
    for name, pb in batches:
        dev = DeviceBatch(pb, p, "cuda:0", audit=pb.n_windows, audit_seed=mld)
        assert dev.n_skipped == 0 and len(dev.audit.chosen) == pb.n_windows, name
        rep = audited(dev)
        launched = {ps.kernel_name(r) for r in capi.launch_log()}
        builds |= launched
        shapes |= {(r["K"], r["pairs_per_wave"]) for r in capi.launch_log()}
        assert rep["n_diff"] == 0, "maxLengthDel %d, %s (%s): %r" % (mld, name, sorted(launched), rep["records"][:3])
        assert rep["n_pairs"] == pb.n_pairs and rep["compared"]["hpos"] > 0, name
    print("audit, maxLengthDel %d: %d builds agree with dd_long_kernel: %s" % (mld, len(builds), ", ".join(sorted(builds))))
    # every build the grid is meant to reach was launched (and so audited).  maxLengthDel <= 11: every lane tiling of the haplotype classes
    # (capi.HAP_CLASSES: positions per lane, pairs per wavefront); at the default maxLengthDel besides, the builds the launch-shape fixture
    # records for these recipes by name.  maxLengthDel 20 runs the one D = 32 build per tiling, whose table is plan.cpp's own: the nine
    # distinct K of the classes up to 574 bp bound it from below whether or not the half-wave tilings exist there.
    if mld <= 11:
        assert shapes >= {(c[2], c[1]) for c in capi.HAP_CLASSES}, sorted(shapes)
    else:
        assert len({k for k, _g in shapes}) >= 9 and all(", 32, " in b for b in builds), sorted(builds)
    if mld == 5:
        assert builds >= {cases[name]["kernel_name"] for name in BUILD_RECIPES}, sorted(builds)


def test_planted_differences_are_named_exactly(lib):
    import torch
    from dindel_tgi_amd.device import DeviceBatch
    pb, index, p, want = ac.scenario()
    dev = DeviceBatch(pb, p, "cuda:0", audit=4, audit_seed=9, audit_max_records=64)
    smp = dev.audit
    assert len(smp.chosen) == 4
    assert audited(dev)["n_diff"] == 0
    st = np.asarray(want["status"])[:pb.n_pairs]
    in_sample = np.isin(ac.window_of_pairs(pb), smp.chosen)
    elem = ps.element_pairs(pb)
    ok = np.nonzero(in_sample & (st == capi.DD_PAIR_OK))[0]
    with_var = np.unique(elem["var_fcov"][:pb.var_cov_len])
    pv = int(ok[np.isin(ok, with_var)][0])
    p_ll, p_hp, p_st = [int(v) for v in ok[~np.isin(ok, [pv])][[0, 5, 9]]]
    outside = int(np.nonzero(~in_sample & (st == capi.DD_PAIR_OK))[0][0])
    e_hp = int(np.nonzero(elem["hpos"][:pb.hpos_len] == p_hp)[0][-1])
    e_vf = int(np.nonzero(elem["var_fcov"][:pb.var_cov_len] == pv)[0][0])
    before = {k: dev.out[k].clone() for k in ("ll", "hpos", "var_fcov", "status")}
    ll_bits = dev.out["ll"].view(torch.int64)
    ll_bits[p_ll] ^= 1 << 52
    ll_bits[outside] ^= 1 << 52
    ll_bits[p_st] ^= 1                                                   # hidden behind this pair's status difference
    dev.out["hpos"][e_hp] ^= 0x100
    dev.out["var_fcov"][e_vf] ^= 1
    dev.out["status"][p_st] ^= 2
    torch.cuda.synchronize()
    dev.launch_audit()
    rep = dev.audit_results()
    got = sorted((r["field"], r["pair"], r["index"], r["primary_bits"] ^ r["shadow_bits"]) for r in rep["records"])
    assert got == sorted([("ll", p_ll, p_ll, 1 << 52), ("hpos", p_hp, e_hp, 0x100), ("var_fcov", pv, e_vf, 1), ("status", p_st, p_st, 2)]), rep["records"]
    assert rep["n_diff"] == 4 and rep["diff"] == dict({k: 0 for k in capi.AUDIT_FIELDS}, ll=1, hpos=1, var_fcov=1, status=1)
    w_of = ac.window_of_pairs(pb)
    assert all(r["window"] == int(w_of[r["pair"]]) for r in rep["records"])
    for r in rep["records"]:
        if r["field"] == "ll":
            assert r["shadow_bits"] == int(np.asarray(want["ll"][p_ll:p_ll + 1]).view(np.uint64)[0])
    # a record cap below the number of differences: the counts stay exact
    dev2 = DeviceBatch(pb, p, "cuda:0", audit=4, audit_seed=9, audit_max_records=1)
    dev2.launch()
    for k, v in before.items():
        dev2.out[k].copy_(dev.out[k])
    torch.cuda.synchronize()
    dev2.launch_audit()
    rep2 = dev2.audit_results()
    assert rep2["n_diff"] == 4 and len(rep2["records"]) == 1 and rep2["diff"] == rep["diff"]


class GuardedShadow:
    """The shadow tensors and the report of a DeviceBatch inside guards, the shadow's bodies poisoned (tests/_output_ownership.GuardedDevice
    does the same for the primary)."""

    def __init__(self, dev):
        import torch
        from dindel_tgi_amd.device import _TORCH_DT
        self.dev, self.raw = dev, {}
        for k in list(dev.shadow):
            dt = np.dtype(RESULT_DTYPES[k])
            nbytes = max(dev._shadow_n[k], 1) * dt.itemsize
            raw = torch.full((nbytes + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev.device)
            raw[GUARD:GUARD + nbytes].fill_(SHADOW_POISON)
            self.raw[k] = raw
            dev.shadow[k] = raw[GUARD:GUARD + nbytes].view(_TORCH_DT[dt])
            setattr(dev.dshadow, k, dev.shadow[k].data_ptr())
        nbytes = dev.audit_report_t.numel() * 8
        raw = torch.full((nbytes + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev.device)
        self.raw["report"] = raw
        dev.audit_report_t = raw[GUARD:GUARD + nbytes].view(torch.int64)
        torch.cuda.synchronize(dev.device)

    def check(self):
        for k, raw in self.raw.items():
            g = raw.cpu().numpy()
            assert (g[:GUARD] == GUARD_BYTE).all() and (g[-GUARD:] == GUARD_BYTE).all(), "the guard around the audit's %s was written" % k


def test_nothing_but_the_owned_shadow_and_the_report_is_written(lib):
    import torch
    from dindel_tgi_amd.device import DeviceBatch
    pb, index, p, want = ac.scenario()
    plain = DeviceBatch(pb, p, "cuda:0")
    gp = GuardedDevice(plain)
    plain.launch()
    torch.cuda.synchronize()
    without = {k: raw.cpu().numpy().copy() for k, raw in gp.raw.items()}

    dev = DeviceBatch(pb, p, "cuda:0", audit=pb.n_windows, audit_seed=2)
    g = GuardedDevice(dev)
    gs = GuardedShadow(dev)
    dev.launch()
    torch.cuda.synchronize()
    before = {k: raw.cpu().numpy().copy() for k, raw in g.raw.items()}
    dev.launch_audit()
    rep = dev.audit_results()
    assert rep["n_diff"] == 0
    g.check("primary after the audit")
    gs.check()
    for k, raw in g.raw.items():
        after = raw.cpu().numpy()
        assert after.tobytes() == before[k].tobytes(), "the audit wrote the primary's %s" % k
        assert after.tobytes() == without[k].tobytes(), "%s differs from a run without audit" % k
    exp, mask = owned_shadow(pb, dev.audit, want)
    for k, m in mask.items():
        got = rep["shadow"][k]
        raw = got.view(np.uint8).reshape(len(got), -1)
        assert (raw[~m] == SHADOW_POISON).all(), "shadow %s: an element outside the rule was written" % k
        assert (raw[m] == exp[k].view(np.uint8).reshape(len(got), -1)[m]).all(), k


def test_more_audited_pairs_than_resident_workgroups(lib):
    from dindel_tgi_amd.device import DeviceBatch
    pb = synth.generate(24, H=4, R=16, L=36, hap_len=100, seed=3)
    p = capi.params_cli_defaults()
    dev = DeviceBatch(pb, p, "cuda:0", audit=pb.n_windows)
    rep = audited(dev)
    log = capi.audit_last_launch()
    assert rep["n_diff"] == 0 and rep["n_pairs"] == pb.n_pairs == log["pairs"]
    assert log["pairs"] > log["grid"] and log["max_pairs_per_wg"] >= 2, log


def test_a_stream_of_its_own_and_a_second_launch_into_the_same_buffers(lib):
    import torch
    from dindel_tgi_amd.device import DeviceBatch
    pb = synth.generate(10, H=3, R=12, L=50, hap_len=120, seed=4)
    p = capi.params_cli_defaults()
    dev = DeviceBatch(pb, p, "cuda:0", audit=5, audit_seed=6)
    st = torch.cuda.Stream(device=dev.device)
    reports = []
    for _ in range(2):
        dev.launch(stream=st)
        dev.launch_audit(stream=st)
        st.synchronize()
        reports.append(dev.audit_results())
    for rep in reports:
        assert rep["n_diff"] == 0 and rep["n_pairs"] == dev.audit.sizes.n_pairs > 0
    assert reports[0]["compared"] == reports[1]["compared"]              # the report is zeroed by each audit, not added to
    for k in reports[0]["shadow"]:
        assert reports[0]["shadow"][k].tobytes() == reports[1]["shadow"][k].tobytes()


def test_long_windows_beside_the_audit(lib):
    import torch
    from dindel_tgi_amd.device import DeviceBatch
    pb = synth.concat([synth.generate(3, H=3, R=8, L=36, hap_len=120, seed=21), synth.generate(1, H=2, R=4, L=36, hap_len=900, seed=22),
                       synth.generate(2, H=2, R=8, L=50, hap_len=200, seed=23)])
    p = ps.params_for(5, 0)
    dev = DeviceBatch(pb, p, "cuda:0", long_windows=True, audit=pb.n_windows)
    cls, _mx, _n = capi.screen_windows_ex(p, pb, capi.DD_OPT_LONG_WINDOWS)
    assert dev.n_long > 0 and list(dev.audit.chosen) == [int(w) for w in np.nonzero(cls == capi.DD_WIN_MAIN)[0] if pb.win_pair_off[w + 1] > pb.win_pair_off[w]]
    dev.launch()
    torch.cuda.synchronize()
    long_log = capi.long_launch_log()
    dev.launch_audit()
    rep = dev.audit_results()
    assert rep["n_diff"] == 0 and rep["n_pairs"] == dev.audit.sizes.n_pairs > 0
    assert capi.long_launch_log() == long_log and len(long_log) == 1       # the likelihood call's log is what it was
    assert capi.audit_last_launch()["pairs"] == rep["n_pairs"]
    # the host-pointer entry with DD_OPT_LONG_WINDOWS: the long window's own launch and the audit's on one stream, each with its workspace
    from dindel_tgi_amd.batch import alloc_result
    b = pb.ctypes_batch()
    plain, res0 = alloc_result(pb)
    assert lib.dd_compute_likelihoods_ex(C.byref(p), C.byref(b), C.byref(res0), 0, capi.DD_OPT_LONG_WINDOWS) == 0, capi.last_error()
    log0 = capi.long_launch_log()
    arrs, res = alloc_result(pb)
    buf = capi.audit_report_buffer(8)
    rc = lib.dd_compute_likelihoods_audit(C.byref(p), C.byref(b), C.byref(res), 0, capi.DD_OPT_LONG_WINDOWS, 3, pb.n_windows, buf.ctypes.data, 8)
    assert rc == 0, capi.last_error()
    hrep = capi.audit_report(buf, 8)
    assert hrep["n_diff"] == 0 and hrep["n_pairs"] == rep["n_pairs"] and hrep["compared"] == rep["compared"]
    assert capi.long_launch_log() == log0 and len(log0) == 1 and log0[0]["pairs"] == long_log[0]["pairs"]
    for k, _t in capi.RESULT_FIELDS:
        assert arrs[k].tobytes() == plain[k].tobytes(), "%s differs from dd_compute_likelihoods_ex" % k
    assert (plain["status"][int(pb.win_pair_off[3]):int(pb.win_pair_off[4])] == capi.DD_PAIR_OK).all()      # the long window was computed
    assert not buf[C.sizeof(capi.dd_audit_report):].any()                                                # unused record slots come back zero


def test_host_pointer_entry_over_two_window_blocks(lib):
    from dindel_tgi_amd.batch import alloc_result
    case = {c["name"]: c for c in ls.load_cases()}["one_shot_two_chunks"]
    pb, _bases = ls.build_batch(case["recipe"])
    p = ls.params_of(case)
    b = pb.ctypes_batch()
    plain, res0 = alloc_result(pb)
    assert lib.dd_compute_likelihoods_ex(C.byref(p), C.byref(b), C.byref(res0), 0, 0) == 0, capi.last_error()
    assert len(capi.launch_log()) == 2                                   # two window blocks
    want_n = 6
    smp = capi.AuditSample(p, pb, want_n, seed=77)
    half = pb.n_windows // 2
    assert (smp.chosen < half).any() and (smp.chosen >= half).any()

    def call(inject=None):
        arrs, res = alloc_result(pb)
        buf = capi.audit_report_buffer(8)
        if inject is not None:
            lib.dd_audit_inject_next(int(inject))
        rc = lib.dd_compute_likelihoods_audit(C.byref(p), C.byref(b), C.byref(res), 0, 0, 77, want_n, buf.ctypes.data, 8)
        assert rc == 0, capi.last_error()
        return arrs, capi.audit_report(buf, 8)
    arrs, rep = call()
    assert len(capi.launch_log()) == 2
    assert rep["n_diff"] == 0 and rep["n_pairs"] == smp.sizes.n_pairs and rep["compared"]["hpos"] == smp.sizes.hpos_len
    for k, _t in capi.RESULT_FIELDS:
        assert arrs[k].tobytes() == plain[k].tobytes(), "%s differs from the call without audit" % k
    # the test hook: one bit of the device copy of ll of a chosen window's first pair, in front of that window's audit
    w = int(smp.chosen[-1])
    arrs, rep = call(inject=w)
    first = int(pb.win_pair_off[w])
    assert rep["n_diff"] == 1 and rep["diff"]["ll"] == 1, rep
    r = rep["records"][0]
    assert (r["window"], r["field"], r["pair"], r["primary_bits"] ^ r["shadow_bits"]) == (w, "ll", first, 1)
    for k, _t in capi.RESULT_FIELDS:
        assert arrs[k].tobytes() == plain[k].tobytes(), "%s: the hook reached the caller's results" % k
    arrs, rep = call()                                                   # the hook is spent
    assert rep["n_diff"] == 0
