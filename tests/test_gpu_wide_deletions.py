"""GPU: wide deletions (DD_OPT_WIDE_DELETIONS, maxLengthDel above 31) — the wide build of the long-window kernel against the CPU oracle,
every dd_result field bit-equal, on both entries, into poisoned and guarded buffers (tests/_output_ownership.py).

Every case first reads from the ORACLE's hpos that the deletion it is about is on a MAP path (tests/_wide_cases.py): compared values alone
would pass on a kernel that never stores a jump of more than 32 states.

Case (c) is about deletions next to the haplotype's ends.  A deletion that itself starts at haplotype base 1 — a one-base flank — is
never on a MAP path: the flank is cheaper as an insertion (about -11.5 - 0.5 n for n inserted bases against -11.5 - 0.5 (y - 1) for y deleted
ones), so a deletion needs flanks longer than itself.  The reads of (c) therefore have their ALIGNMENT start at base 1 / end at the last
base, with the deletion behind / in front of a 55-bp flank; checked on the oracle before any kernel result is looked at.
"""
import ctypes as C
from unittest import mock

import numpy as np
import pytest

from dindel_tgi_amd import capi
from tests import _output_ownership as oo
from tests import _wide_cases as wc

pytestmark = pytest.mark.gpu
WIDE = capi.DD_OPT_LONG_WINDOWS | capi.DD_OPT_WIDE_DELETIONS


def ownership(pb, want, p, faster=False):
    """tests/_output_ownership.must_write with the unsupported windows of THIS screen (the wide one: every window within the long limits is
    computed), not dd_screen_windows'."""
    if faster:
        return oo.must_write(pb, want, faster=True)
    cls, _mx, _n = capi.screen_windows_ex(p, pb, WIDE)
    unsup = np.zeros(pb.n_pairs, bool)
    for w in np.nonzero(cls == capi.DD_WIN_UNSUPPORTED)[0]:
        unsup[int(pb.win_pair_off[w]):int(pb.win_pair_off[w + 1])] = True
    with mock.patch.object(oo, "unsupported_pairs", lambda _pb: unsup):
        return oo.must_write(pb, want)


def host_wide(lib, p, pb, options=WIDE):
    arrs, res = oo.alloc_poisoned(pb)
    b = pb.ctypes_batch()
    with oo.poisoned_arena():
        rc = lib.dd_compute_likelihoods_ex(C.byref(p), C.byref(b), C.byref(res), 0, options)
    assert rc == 0, capi.last_error()
    return arrs


def device_wide(p, pb, stream=None, **kw):
    """DeviceBatch(long_windows, wide_deletions) with poisoned, guarded result tensors -> (results, batch, guards)."""
    import torch
    from dindel_tgi_amd.device import DeviceBatch
    dev = DeviceBatch(pb, p, "cuda:0", long_windows=True, wide_deletions=True, **kw)
    g = oo.GuardedDevice(dev)
    dev.launch(stream)
    torch.cuda.synchronize()
    return dev.results(), dev, g


def check_both(lib, p, pb, want, where, K=None):
    """Both entries against the oracle -> the device entry's launch record."""
    own = ownership(pb, want, p)
    got, _dev, g = device_wide(p, pb)
    log = capi.long_launch_log()
    oo.assert_owned(got, want, pb, own, where + ", device-pointer path")
    g.check(where + ", device-pointer path")
    assert len(log) == 1 and log[0]["wide"], log
    if K is not None:
        assert log[0]["K"] == K, log
    oo.assert_owned(host_wide(lib, p, pb), want, pb, own, where + ", host-pointer path")
    hlog = capi.long_launch_log()
    assert len(hlog) == 1 and hlog[0]["wide"] and hlog[0]["K"] == log[0]["K"], hlog
    return log[0]


# ---- (a) boundaries of the field ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mld", wc.A_MLDS)
def test_field_boundaries(lib, mld):
    pb, p = wc.case_a(), wc.params(mld)
    want = wc.oracle("case_a", mld)
    st = want["status"][:pb.n_pairs]
    planted = [wc.longest_deletion(pb, want, 0, 0, r) for r in range(4)]
    if mld == 201:
        assert (st == capi.DD_PAIR_HAPSIZE).all()
    elif mld < 40:
        assert max(planted) < 40, planted                       # the deletion does not fit: absent
    else:
        assert planted == [40] * 4, planted                       # on the MAP path of each of the four reads
        assert (st[:12] == capi.DD_PAIR_OK).all()
    if mld == 200:
        assert (st[12:] == capi.DD_PAIR_HAPSIZE).all()            # the 197- and 199-bp haplotypes
    check_both(lib, p, pb, want, "(a) maxLengthDel %d" % mld, K=1)


def test_default_pfirstglo_places_the_read_off_the_haplotype(lib):
    """At the default pFirstgLO the same reads carry no deletion: the option then changes the hapSize status and nothing else."""
    pb, p = wc.case_a(), wc.params(45, 0.01)
    want = wc.oracle("case_a", 45, 0.01)
    assert [wc.longest_deletion(pb, want, 0, 0, r) for r in range(4)] == [0] * 4
    check_both(lib, p, pb, want, "(a) default pFirstgLO")


# ---- (b) crossing 6 bits and 8 bits ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mld", [69, 70, 100])
def test_seventy_base_deletion(lib, mld):
    pb, p = wc.case_b70(), wc.params(mld)
    want = wc.oracle("case_b70", mld)
    found = [wc.longest_deletion(pb, want, 0, 0, r) for r in (0, 2)]
    assert found == ([70, 70] if mld >= 70 else [0, 0]), found    # 70 is the exact boundary; at 69 the flank is inserted instead
    check_both(lib, p, pb, want, "(b) 70 bp, maxLengthDel %d" % mld, K=2)


def test_260_base_deletion(lib):
    pb, p = wc.case_b260(), wc.params(300)
    want = wc.oracle("case_b260", 300)
    assert wc.deletions_of(wc.pair_hpos(pb, want, 0, 0, 0)) == [(300, 260)] and wc.deletions_of(wc.pair_hpos(pb, want, 0, 0, 2)) == [(290, 260)]
    check_both(lib, p, pb, want, "(b) 260 bp", K=4)


# ---- (c) K builds and clipping --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hs,K", [(254, 1), (255, 2)])
def test_k_builds_and_haplotype_ends(lib, hs, K):
    pb, p = wc.case_c(hs), wc.params(64, 0.5)
    want = wc.oracle("case_c", 64, 0.5, False, hs)
    F = wc.C_FLANK
    rows = [wc.pair_hpos(pb, want, 0, 0, r) for r in range(5)]

    def one(row, at, n):      # one deletion of n bases, placed where it was planted (or a base or two beside it, where the bases repeat)
        d = wc.deletions_of(row)
        return len(d) == 1 and d[0][1] == n and abs(d[0][0] - at) <= 2
    assert one(rows[0], F, 40) and rows[0][0] == 0                                          # the alignment starts at haplotype base 1
    assert one(rows[1], hs - F - 40, 40) and rows[1][-1] == hs - 1                          # ... ends at the last base
    assert one(rows[2], F, 40) and (rows[2][:20] == capi.DD_HPOS_LO).all()
    assert one(rows[3], hs - F - 40, 40) and (rows[3][-20:] == capi.DD_HPOS_RO).all()
    assert one(rows[4], 100, 50)
    check_both(lib, p, pb, want, "(c) %d bp" % hs, K=K)


def test_max_length_del_equal_to_the_haplotype(lib):
    pb, p = wc.case_c40(), wc.params(40, 0.5)
    want = wc.oracle("case_c40", 40, 0.5)
    st = want["status"][:pb.n_pairs]
    assert (st[:4] == capi.DD_PAIR_OK).all() and (st[4:] == capi.DD_PAIR_HAPSIZE).all()     # the 39-bp haplotype
    assert wc.deletions_of(wc.pair_hpos(pb, want, 0, 0, 2)) == [(15, 10)]
    check_both(lib, p, pb, want, "(c) maxLengthDel = Hs = 40", K=1)


# ---- (d) ties over many equal candidates ----------------------------------------------------------------------------------------
def test_tandem_repeat_ties(lib):
    pb, p = wc.case_d(), wc.params(64)
    want = wc.oracle("case_d", 64)
    for i, n_del in enumerate(wc.D_DELS):
        d = wc.deletions_of(wc.pair_hpos(pb, want, 0, 0, 2 * i))
        assert len(d) == 1 and d[0][1] == n_del and 60 <= d[0][0] <= 300 - n_del, (n_del, d)
    check_both(lib, p, pb, want, "(d) tandem repeat", K=2)


# ---- (e) later items of a workgroup, and placeholders ---------------------------------------------------------------------------
def test_more_pairs_than_the_grid_and_placeholders(lib):
    pb, p = wc.case_e(), wc.params(40)
    want = wc.oracle("case_e", 40)
    cls, _mx, n_bad = capi.screen_windows_ex(p, pb, WIDE)
    assert list(cls) == [2, 2, 2, 2, 1, 1, 2] and n_bad == 2
    rec = check_both(lib, p, pb, want, "(e)")
    assert rec["pairs"] == 640 and rec["grid"] < 640 and rec["max_pairs_per_wg"] >= 2, rec
    # the placeholders and onHap once more by hand, from the device entry
    got, _dev, _g = device_wide(p, pb)
    for w in (4, 5):
        ps = slice(int(pb.win_pair_off[w]), int(pb.win_pair_off[w + 1]))
        assert ps.stop > ps.start
        assert (got["status"][ps] == capi.DD_PAIR_UNSUPPORTED).all() and (got["ll"][ps] == 0).all()
        assert (got["offHap"][ps] == 1).all() and (got["offHapHMQ"][ps] == 1).all()
    ro = pb.a["win_read_off"]
    assert not got["onHap"][int(ro[4]):].any() and got["onHap"][:int(ro[4])].any()
    assert np.array_equal(got["onHap"][:int(ro[4])], want["onHap"][:int(ro[4])])


def test_a_batch_without_any_long_window(lib):
    """Every window beyond the long limits: no kernel launch, the placeholders and onHap still come from the wide launch."""
    from dindel_tgi_amd.batch import Window, pack
    rng = np.random.default_rng(4350)
    pb = pack([Window(wc.S, [wc.rnd(rng, 4500)], [wc.plain_read(wc.rnd(rng, 100), 0, 60), wc.plain_read(wc.rnd(rng, 100), 0, 50)])])
    p = wc.params(40)
    got, _dev, g = device_wide(p, pb)
    g.check("no long window")
    assert (got["status"] == capi.DD_PAIR_UNSUPPORTED).all() and (got["ll"] == 0).all() and (got["offHap"] == 1).all()
    assert (got["onHap"] == 0).all()
    assert (np.ascontiguousarray(got["hpos"]).view(np.uint8) == oo.BODY_BYTE).all()
    host = host_wide(lib, p, pb)
    assert (host["status"][:2] == capi.DD_PAIR_UNSUPPORTED).all() and (host["onHap"][:2] == 0).all()


# ---- (f) the --faster entries ----------------------------------------------------------------------------------------------------
def test_faster_entries_take_the_bit(lib):
    from dindel_tgi_amd.device import DeviceBatch
    import torch
    pb, p = wc.case_f(), wc.params(40, 0.01)
    want = wc.oracle("case_f", 40, 0.01, True)
    st = want["status"][:pb.n_pairs]
    R = pb.n_reads
    assert (st[2 * R:] == capi.DD_PAIR_HAPSIZE).all() and (st[:2 * R] == capi.DD_PAIR_OK).all()     # the 30-bp haplotype
    own = ownership(pb, want, p, faster=True)
    b = pb.ctypes_batch()
    arrs, res = oo.alloc_poisoned(pb)
    assert lib.dd_compute_likelihoods_faster_ex(C.byref(p), C.byref(b), C.byref(res), 0, 0) == capi.DD_ERR_UNSUPPORTED
    with oo.poisoned_arena():
        rc = lib.dd_compute_likelihoods_faster_ex(C.byref(p), C.byref(b), C.byref(res), 0, capi.DD_OPT_WIDE_DELETIONS)
    assert rc == 0, capi.last_error()
    oo.assert_owned(arrs, want, pb, own, "(f) dd_compute_likelihoods_faster_ex")
    arrs, res = oo.alloc_poisoned(pb)
    keys = np.zeros(max(pb.n_pairs, 1), np.int16)
    with oo.poisoned_arena():
        rc = lib.dd_compute_likelihoods_faster_keys(C.byref(p), C.byref(b), C.byref(res), keys.ctypes.data_as(capi.c_i16p), 0,
                                                    capi.DD_OPT_WIDE_DELETIONS | capi.DD_OPT_LONG_WINDOWS_FASTER)
    assert rc == 0, capi.last_error()
    oo.assert_owned(arrs, want, pb, own, "(f) dd_compute_likelihoods_faster_keys")
    assert np.array_equal(keys[:pb.n_pairs], capi.indel_keys_host(pb, want["hpos"], want["status"]))
    with pytest.raises(RuntimeError, match="maxLengthDel"):
        DeviceBatch(pb, p, "cuda:0")
    dev = DeviceBatch(pb, p, "cuda:0", wide_deletions_faster=True)
    g = oo.GuardedDevice(dev)
    dev.launch_faster()
    torch.cuda.synchronize()
    oo.assert_owned(dev.results(), want, pb, own, "(f) dd_launch_device_faster_ex")
    g.check("(f) dd_launch_device_faster_ex")


# ---- (g) device-pointer path -----------------------------------------------------------------------------------------------------
def test_device_path_on_a_stream_twice_then_cigars(lib):
    import torch
    from tests import _cigar_cases as cc
    pb, p = wc.case_b260(), wc.params(300)
    want = wc.oracle("case_b260", 300)
    own = ownership(pb, want, p)
    hrp = cc.batch_hap_ref_pos(pb, 77)
    st = torch.cuda.Stream(device="cuda:0")
    got, dev, g = device_wide(p, pb, stream=st, cigars=True, ops_cap=8, hap_ref_pos=hrp)
    oo.assert_owned(got, want, pb, own, "(g) first launch on a stream of its own")
    before = {k: t.cpu().numpy().copy() for k, t in g.raw.items()}
    dev.launch(st)                                                          # the same tensors, not poisoned again
    torch.cuda.synchronize()
    after = {k: t.cpu().numpy().copy() for k, t in g.raw.items()}
    for k in before:
        assert np.array_equal(before[k], after[k]), "second launch into the same tensors: %s changed" % k
    fill = 0x3B3B3B3B
    for t in dev.cig.values():
        t.fill_(fill)
    dev.launch_cigars(st)
    res = dev.results()
    cig = {k: res["cigar_" + k] for k in ("n_ops", "ops", "ref_off", "status")}
    exp, outcomes = cc.expected(pb, want["hpos"], hrp, None, want["status"][:pb.n_pairs], 8, fill)
    cc.assert_equal(cig, exp, outcomes)
    assert wc.deletions_of(wc.pair_hpos(pb, want, 0, 0, 0)) == [(300, 260)]
    assert isinstance(outcomes[0], tuple) and any(op == cc.D and ln >= 260 for op, ln in outcomes[0][0]), outcomes[0]


def test_wide_deletions_needs_long_windows():
    from dindel_tgi_amd.device import DeviceBatch
    with pytest.raises(ValueError, match="long_windows"):
        DeviceBatch(wc.case_a(), wc.params(40), "cuda:0", wide_deletions=True)
    # with maxLengthDel <= 31 the flag changes nothing: the main launch, then the long launch where there are long windows
    p = wc.params(31)
    pb = wc.case_a()
    dev = DeviceBatch(pb, p, "cuda:0", long_windows=True, wide_deletions=True)
    assert not dev.wide and dev.n_long == 0
    dev.launch()
    got = dev.results()
    want = wc.oracle("case_a", 31)
    for k, _t in capi.RESULT_FIELDS:
        assert got[k].tobytes() == want[k][:len(got[k])].tobytes(), k
