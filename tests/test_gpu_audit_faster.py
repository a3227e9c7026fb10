"""The audit of the --faster model on the device: a sample of a --faster launch's windows recomputed by the independent shadow kernel
(csrc/faster_shadow_kernel.hip, the model of csrc/faster_shadow.h) and compared, bit for bit, with what dd_faster_kernel and
dd_faster_long_kernel left in HBM (dd_audit_device_faster, DeviceBatch(audit_faster=N)).

  clean      every eligible window of two scenario batches, at 4, 2 and 1 pairs per wavefront of dd_faster_kernel: no difference, the shadow
             bit-equal to the oracle on every element the rule names, the elements compared per field equal to numpy's own count
  planted    bits inverted through torch in every field of audited pairs, a status, and ll of a pair outside the sample: the report names
             exactly the planted ones
  guards     256-byte guards around primary, shadow, report and workspace, different poison in primary and shadow: nothing but the shadow's
             owned elements and the report is written, and the primary is byte-identical before and after
  variants   more audited pairs than the persistent grid has wavefronts; a stream of its own with a second launch into the same buffers;
             the two smallest long windows (767-bp haplotype, 1,025-bp read: the HBM workspace) beside ordinary ones"""
import ctypes as C

import numpy as np
import pytest

from dindel_tgi_amd import capi, synth
from dindel_tgi_amd.batch import RESULT_DTYPES
from tests import _audit_cases as ac
from tests import _audit_faster_cases as fc
from tests import _path_scenarios as ps
from tests._output_ownership import GUARD, GUARD_BYTE, GuardedDevice

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return capi.load()


def audited(dev):
    """launch_faster(), launch_audit_faster() -> the report (with shadow and sample)."""
    dev.launch_faster()
    dev.launch_audit_faster()
    return dev.audit_faster_results()


@pytest.mark.parametrize("groups", [4, 2, 1])
@pytest.mark.parametrize("shape", [(126, 36, 5), (30, 100, 11)])
def test_clean_audit_of_every_eligible_window(lib, monkeypatch, shape, groups):
    from dindel_tgi_amd.device import DeviceBatch
    if groups != 4:
        monkeypatch.setenv("DD_FAST_GROUPS", str(groups))
    else:
        monkeypatch.delenv("DD_FAST_GROUPS", raising=False)
    pb, index, p, want = fc.scenario(*shape)
    dev = DeviceBatch(pb, p, "cuda:0", audit_faster=pb.n_windows, audit_seed=1)
    smp = dev.audit_faster
    assert list(smp.chosen) == list(fc.eligible_windows(pb, fc.faster_classes(p, pb))) and 0 < len(smp.chosen) < pb.n_windows
    rep = audited(dev)
    shape_rec = (C.c_int32 * 8)()
    lib.dd_last_launch(C.byref(shape_rec))
    assert int(shape_rec[0]) == groups                                   # pairs per wavefront of the dd_faster_kernel launch that was audited
    assert rep["n_diff"] == 0 and not any(rep["diff"].values()), rep["records"][:5]
    assert rep["n_pairs"] == smp.sizes.n_pairs
    exp, mask = fc.owned_shadow(pb, smp, want)
    fc.assert_shadow_is_the_oracles(rep["shadow"], exp, mask)
    assert rep["compared"] == fc.expected_compared(pb, want["status"], smp.chosen, True)
    st = np.asarray(want["status"])[:pb.n_pairs]
    assert all((st == s).any() for s in (capi.DD_PAIR_OK, capi.DD_PAIR_NAN, capi.DD_PAIR_HAPSIZE))
    log = capi.audit_last_launch_faster()
    assert log["pairs"] == smp.sizes.n_pairs and log["in_lds"] == 1 and log["ws_bytes"] == 0 and log["grid"] > 0 and log["compare_grid"] > 0, log
    assert (log["max_hap"], log["max_read"]) == (smp.sizes.max_hap_len, smp.sizes.max_read_len)


def test_planted_differences_are_named_exactly(lib):
    import torch
    from dindel_tgi_amd.device import DeviceBatch
    pb, index, p, want = fc.scenario()
    dev = DeviceBatch(pb, p, "cuda:0", audit_faster=5, audit_seed=9, audit_max_records=64)
    smp = dev.audit_faster
    assert len(smp.chosen) == 5
    assert audited(dev)["n_diff"] == 0
    st = np.asarray(want["status"])[:pb.n_pairs]
    in_sample = np.isin(ac.window_of_pairs(pb), smp.chosen)
    elem = ps.element_pairs(pb)
    ok = np.nonzero(in_sample & (st == capi.DD_PAIR_OK))[0]
    with_var = np.unique(elem["var_fcov"][:pb.var_cov_len])
    pv = int(ok[np.isin(ok, with_var)][0])
    rest = ok[~np.isin(ok, [pv])]
    assert len(rest) >= 16
    p_st = int(rest[15])
    outside = int(np.nonzero(~in_sample & (st == capi.DD_PAIR_OK))[0][0])
    bits_of = {8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.uint8}
    planted = []
    for i, k in enumerate(capi.AUDIT_FIELDS[1:15]):                       # one bit in each per-pair value, each in a pair of its own
        pair = int(rest[i])
        dev.out[k].view(bits_of[dev.out[k].element_size()])[pair] ^= 4
        planted.append((k, pair, pair, 4))
    e_hp = int(np.nonzero(elem["hpos"][:pb.hpos_len] == int(rest[3]))[0][-1])
    dev.out["hpos"][e_hp] ^= 0x100
    planted.append(("hpos", int(rest[3]), e_hp, 0x100))
    e_vc, e_vf = (int(np.nonzero(elem["var_fcov"][:pb.var_cov_len] == pv)[0][i]) for i in (0, -1))
    dev.out["var_covered"][e_vc] ^= 1
    dev.out["var_fcov"][e_vf] ^= 1
    planted += [("var_covered", pv, e_vc, 1), ("var_fcov", pv, e_vf, 1)]
    dev.out["status"][p_st] ^= 2
    dev.out["ll"].view(torch.int64)[p_st] ^= 1                           # hidden behind this pair's status difference
    planted.append(("status", p_st, p_st, 2))
    dev.out["ll"].view(torch.int64)[outside] ^= 1 << 52                  # a window the sample does not hold
    torch.cuda.synchronize()
    dev.launch_audit_faster()
    rep = dev.audit_faster_results()
    got = sorted((r["field"], r["pair"], r["index"], r["primary_bits"] ^ r["shadow_bits"]) for r in rep["records"])
    assert got == sorted(planted), rep["records"]
    assert rep["n_diff"] == len(planted) and sum(rep["diff"].values()) == len(planted)
    w_of = ac.window_of_pairs(pb)
    assert all(r["window"] == int(w_of[r["pair"]]) for r in rep["records"])


class GuardedShadow:
    """The shadow tensors, the report and the workspace of a DeviceBatch(audit_faster=N) inside guards, the shadow's bodies poisoned."""

    def __init__(self, dev):
        import torch
        from dindel_tgi_amd.device import _TORCH_DT
        self.dev, self.raw = dev, {}

        def guarded(nbytes, fill=None):
            raw = torch.full((nbytes + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev.device)
            if fill is not None:
                raw[GUARD:GUARD + nbytes].fill_(fill)
            return raw
        for k in list(dev.shadow_faster):
            dt = np.dtype(RESULT_DTYPES[k])
            nbytes = max(dev._shadow_faster_n[k], 1) * dt.itemsize
            self.raw[k] = guarded(nbytes, fc.SHADOW_POISON)
            dev.shadow_faster[k] = self.raw[k][GUARD:GUARD + nbytes].view(_TORCH_DT[dt])
            setattr(dev.dshadow_faster, k, dev.shadow_faster[k].data_ptr())
        nbytes = dev.audit_faster_report_t.numel() * 8
        self.raw["report"] = guarded(nbytes)
        dev.audit_faster_report_t = self.raw["report"][GUARD:GUARD + nbytes].view(torch.int64)
        nbytes = max(dev.audit_faster_ws_bytes, 8)
        self.raw["workspace"] = guarded(nbytes, 0x77)
        dev.audit_faster_ws = self.raw["workspace"][GUARD:GUARD + nbytes]
        torch.cuda.synchronize(dev.device)

    def check(self):
        for k, raw in self.raw.items():
            g = raw.cpu().numpy()
            assert (g[:GUARD] == GUARD_BYTE).all() and (g[-GUARD:] == GUARD_BYTE).all(), "the guard around the audit's %s was written" % k


def guarded_run(pb, p, want, long_windows):
    import torch
    from dindel_tgi_amd.device import DeviceBatch
    dev = DeviceBatch(pb, p, "cuda:0", long_windows_faster=long_windows, audit_faster=pb.n_windows, audit_seed=2)
    g = GuardedDevice(dev)
    gs = GuardedShadow(dev)
    dev.launch_faster()
    torch.cuda.synchronize()
    before = {k: raw.cpu().numpy().copy() for k, raw in g.raw.items()}
    dev.launch_audit_faster()
    rep = dev.audit_faster_results()
    assert rep["n_diff"] == 0, rep["records"][:5]
    g.check("primary after the audit")
    gs.check()
    for k, raw in g.raw.items():
        assert raw.cpu().numpy().tobytes() == before[k].tobytes(), "the audit wrote the primary's %s" % k
    exp, mask = fc.owned_shadow(pb, dev.audit_faster, want)
    fc.assert_shadow_is_the_oracles(rep["shadow"], exp, mask, fc.SHADOW_POISON)
    return dev, rep


def test_nothing_but_the_owned_shadow_and_the_report_is_written(lib):
    pb, index, p, want = fc.scenario()
    dev, rep = guarded_run(pb, p, want, False)
    assert rep["n_pairs"] == dev.audit_faster.sizes.n_pairs > 0 and dev.audit_faster_ws_bytes == 0


def test_long_windows_are_audited_beside_ordinary_ones(lib):
    pb, p, want = fc.long_scenario()
    dev, rep = guarded_run(pb, p, want, True)
    smp = dev.audit_faster
    assert dev.n_long == 2 and list(smp.chosen) == list(range(pb.n_windows))
    assert (smp.sizes.max_hap_len, smp.sizes.max_read_len) == (771, 1025)
    log = capi.audit_last_launch_faster()
    assert log["in_lds"] == 0 and log["ws_bytes"] == dev.audit_faster_ws_bytes > 0 and log["pairs"] == pb.n_pairs == rep["n_pairs"], log
    assert rep["compared"] == fc.expected_compared(pb, want["status"], smp.chosen, True)
    # without the option the long windows are neither computed nor audited
    from dindel_tgi_amd.device import DeviceBatch
    plain = DeviceBatch(pb, p, "cuda:0", audit_faster=pb.n_windows)
    assert list(plain.audit_faster.chosen) == [0, 3]
    rep = audited(plain)
    assert rep["n_diff"] == 0 and rep["n_pairs"] == plain.audit_faster.sizes.n_pairs and capi.audit_last_launch_faster()["in_lds"] == 1


def test_more_audited_pairs_than_the_grid_has_wavefronts(lib):
    from dindel_tgi_amd.device import DeviceBatch
    pb = synth.generate(33, H=4, R=64, L=36, hap_len=30, seed=3)
    p = capi.params_cli_defaults()
    dev = DeviceBatch(pb, p, "cuda:0", audit_faster=pb.n_windows)
    rep = audited(dev)
    log = capi.audit_last_launch_faster()
    assert pb.n_pairs > 8192 and rep["n_diff"] == 0 and rep["n_pairs"] == pb.n_pairs == log["pairs"], rep["records"][:3]
    assert log["grid"] == 2048 and log["pairs"] > 4 * log["grid"], log
    assert rep["compared"]["hpos"] == pb.hpos_len


def test_a_stream_of_its_own_and_a_second_launch_into_the_same_buffers(lib):
    import torch
    from dindel_tgi_amd.device import DeviceBatch
    pb = synth.generate(10, H=3, R=12, L=50, hap_len=120, seed=4)
    p = capi.params_cli_defaults()
    dev = DeviceBatch(pb, p, "cuda:0", audit_faster=5, audit_seed=6)
    st = torch.cuda.Stream(device=dev.device)
    reports = []
    for _ in range(2):
        dev.launch_faster(stream=st)
        dev.launch_audit_faster(stream=st)
        st.synchronize()
        reports.append(dev.audit_faster_results())
    for rep in reports:
        assert rep["n_diff"] == 0 and rep["n_pairs"] == dev.audit_faster.sizes.n_pairs > 0
    assert reports[0]["compared"] == reports[1]["compared"]              # the report is zeroed by each audit, not added to
    for k in reports[0]["shadow"]:
        assert reports[0]["shadow"][k].tobytes() == reports[1]["shadow"][k].tobytes()


def test_device_batch_arguments(lib):
    from dindel_tgi_amd.device import DeviceBatch
    pb = synth.generate(4, H=2, R=4, L=36, hap_len=60, seed=5)
    p = capi.params_cli_defaults()
    with pytest.raises(ValueError, match="long_windows"):
        DeviceBatch(pb, p, "cuda:0", long_windows=True, audit_faster=2)
    with pytest.raises(ValueError, match="long_windows_faster"):                                   # the main model's audit keeps its refusal
        DeviceBatch(pb, p, "cuda:0", long_windows_faster=True, audit=2)
    with pytest.raises(RuntimeError, match="audit_faster"):
        DeviceBatch(pb, p, "cuda:0").launch_audit_faster()


def host_call(lib, p, pb, keys, options, seed, want_n, inject=None, cap=8):
    """dd_compute_likelihoods_faster_audit -> (result arrays, keys or None, report)"""
    from dindel_tgi_amd.batch import alloc_result
    b = pb.ctypes_batch()
    arrs, res = alloc_result(pb)
    kout = np.full(max(pb.n_pairs, 1), -7, np.int16) if keys else None
    buf = capi.audit_report_buffer(cap)
    buf[...] = 0xEE
    if inject is not None:
        lib.dd_audit_inject_next(int(inject))
    rc = lib.dd_compute_likelihoods_faster_audit(C.byref(p), C.byref(b), C.byref(res), kout.ctypes.data_as(capi.c_i16p) if keys else None, 0, options,
                                                 seed, want_n, buf.ctypes.data, cap)
    assert rc == 0, capi.last_error()
    return arrs, kout, capi.audit_report(buf, cap)


def plain_call(lib, p, pb, keys, options):
    from dindel_tgi_amd.batch import alloc_result
    b = pb.ctypes_batch()
    arrs, res = alloc_result(pb)
    if keys:
        kout = np.full(max(pb.n_pairs, 1), -7, np.int16)
        assert lib.dd_compute_likelihoods_faster_keys(C.byref(p), C.byref(b), C.byref(res), kout.ctypes.data_as(capi.c_i16p), 0, options) == 0, capi.last_error()
        return arrs, kout
    assert lib.dd_compute_likelihoods_faster_ex(C.byref(p), C.byref(b), C.byref(res), 0, options) == 0, capi.last_error()
    return arrs, None


@pytest.mark.parametrize("keys", [False, True])
def test_host_pointer_entry_over_two_window_blocks(lib, keys):
    from tests import _launch_shapes as ls
    case = {c["name"]: c for c in ls.load_cases()}["one_shot_two_chunks"]
    pb, _bases = ls.build_batch(case["recipe"])
    p = ls.params_of(case)
    plain, pkeys = plain_call(lib, p, pb, keys, 0)
    want_n = 6
    smp = capi.AuditSample(p, pb, want_n, seed=77, faster=True)
    half = pb.n_windows // 2
    assert (smp.chosen < half).any() and (smp.chosen >= half).any()
    arrs, kout, rep = host_call(lib, p, pb, keys, 0, 77, want_n)
    assert 0 < capi.audit_last_launch_faster()["pairs"] < smp.sizes.n_pairs   # the record is the last block's: there was more than one
    assert rep["n_diff"] == 0 and rep["n_pairs"] == smp.sizes.n_pairs and rep["compared"]["hpos"] == smp.sizes.hpos_len, rep
    for k, _t in capi.RESULT_FIELDS:
        assert arrs[k].tobytes() == plain[k].tobytes(), "%s differs from the call without audit" % k
    if keys:
        assert kout.tobytes() == pkeys.tobytes()
    # the test hook: one bit of the device copy of ll of a chosen window's first pair, in front of that window's audit
    w = int(smp.chosen[-1])
    arrs, kout, rep = host_call(lib, p, pb, keys, 0, 77, want_n, inject=w)
    first = int(pb.win_pair_off[w])
    assert rep["n_diff"] == 1 and rep["diff"]["ll"] == 1, rep
    r = rep["records"][0]
    assert (r["window"], r["field"], r["pair"], r["primary_bits"] ^ r["shadow_bits"]) == (w, "ll", first, 1)
    for k, _t in capi.RESULT_FIELDS:
        assert arrs[k].tobytes() == plain[k].tobytes(), "%s: the hook reached the caller's results" % k
    arrs, kout, rep = host_call(lib, p, pb, keys, 0, 77, want_n)         # the hook is spent
    assert rep["n_diff"] == 0


def test_host_pointer_entry_with_long_windows_and_without_hpos(lib):
    from dindel_tgi_amd.batch import alloc_result
    pb, p, want = fc.long_scenario()
    opt = capi.DD_OPT_LONG_WINDOWS_FASTER
    plain, _k = plain_call(lib, p, pb, False, opt)
    arrs, _k, rep = host_call(lib, p, pb, False, opt, 3, pb.n_windows)
    assert rep["n_diff"] == 0 and rep["n_pairs"] == pb.n_pairs and rep["compared"] == fc.expected_compared(pb, want["status"], range(pb.n_windows), True)
    for k, _t in capi.RESULT_FIELDS:
        assert arrs[k].tobytes() == plain[k].tobytes(), "%s differs from dd_compute_likelihoods_faster_ex" % k
    assert (plain["status"][:pb.n_pairs] == capi.DD_PAIR_OK).all()       # the long windows were computed
    assert capi.audit_last_launch_faster()["in_lds"] == 0
    _a, _k, rep0 = host_call(lib, p, pb, False, 0, 3, pb.n_windows)      # without the option: the ordinary windows alone
    assert rep0["n_diff"] == 0 and 0 < rep0["n_pairs"] < pb.n_pairs and capi.audit_last_launch_faster()["in_lds"] == 1
    # the key entry without r->hpos: hpos is on the device for the key launch anyway, and is compared
    b = pb.ctypes_batch()
    arrs2, res2 = alloc_result(pb)
    res2.hpos = None
    kout = np.zeros(pb.n_pairs, np.int16)
    buf = capi.audit_report_buffer(4)
    rc = lib.dd_compute_likelihoods_faster_audit(C.byref(p), C.byref(b), C.byref(res2), kout.ctypes.data_as(capi.c_i16p), 0, opt, 3, pb.n_windows,
                                                 buf.ctypes.data, 4)
    assert rc == 0, capi.last_error()
    rep2 = capi.audit_report(buf, 4)
    assert rep2["n_diff"] == 0 and rep2["compared"]["hpos"] == pb.hpos_len and rep2["compared"] == rep["compared"]
    # want 0 and validation
    _a, _k, rep3 = host_call(lib, p, pb, False, opt, 3, 0)
    assert rep3["n_pairs"] == 0 and rep3["n_diff"] == 0
    assert lib.dd_compute_likelihoods_faster_audit(C.byref(p), C.byref(b), C.byref(res2), None, 0, capi.DD_OPT_LONG_WINDOWS, 3, 2, buf.ctypes.data, 4) == capi.DD_ERR_INVALID
    assert lib.dd_compute_likelihoods_faster_audit(C.byref(p), C.byref(b), C.byref(res2), None, 0, 0, 3, 2, None, 4) == capi.DD_ERR_INVALID
