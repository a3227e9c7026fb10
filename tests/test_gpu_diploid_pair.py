"""GPU: the certified MAP haplotype pair on the device (dd_diploid_pairs_device, diploid_pair_kernel.hip) against its CPU evaluation
(dd_diploid_pairs_host, checked against the real host function in tests/test_diploid_pair_cpu.py): every output equal in every bit, on the
windows of tests/_diploid_pair_cases.py — as one batch (more windows than the grid has workgroups), as batches of one window, with 65 and
with the most haplotypes a window may have.  Then the launch chained in front of the realign launch (DD_REALIGN_PAIR) behind the likelihood
launches: certified windows' reads get the row of the per-pair CIGAR launch for the haplotype the diploid rule chooses, every other window's
reads DD_REALIGN_BAD_PAIR."""
import ctypes as C

import numpy as np
import pytest
import torch

from dindel_tgi_amd import capi, synth
from dindel_tgi_amd.batch import pack
from dindel_tgi_amd.device import DeviceBatch
from tests import _cigar_cases as cc
from tests import _diploid_pair_cases as dc
from tests import test_gpu_realign as tgr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = tgr.FILL
GRID = 2048                        # workgroups of the persistent grid (csrc/diploid_pair_kernel.h, kMaxBlocks): one window each per round


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class Resident:
    """build()'s arrays in HBM once, and outputs that start out filled with a pattern."""

    def __init__(self):
        c = dc.build()
        self.c, self.W = c, c["n_windows"]
        up = lambda a: torch.from_numpy(np.array(a)).to(DEV)
        self.t = {k: up(c[k]) for k in ("ho", "ro", "po", "hh", "ll", "prior", "status")}
        self.out = {k: torch.empty(self.W * (2 if k == "pair" else 1), dtype=torch.int32 if k in ("pair", "state") else torch.float64, device=DEV)
                    for k in capi.DIPLOID_PAIR_FIELDS}
        self.reset()

    def reset(self):
        for k, v in self.out.items():
            v.fill_(FILL if v.dtype == torch.int32 else -12345.5)

    def launch(self, lib, w0=0, n=None, status=True):
        """windows [w0, w0 + n) as a batch of their own: the offset arrays and the outputs start at window w0, ll and prior where they are."""
        n = self.W - w0 if n is None else n
        db = capi.dd_device_batch()
        db.n_windows = n
        db.win_hap_off = self.t["ho"].data_ptr() + 4 * w0
        db.win_read_off = self.t["ro"].data_ptr() + 4 * w0
        db.win_pair_off = self.t["po"].data_ptr() + 8 * w0
        o = self.out
        res = capi.dd_diploid_pair_result(o["pair"].data_ptr() + 8 * w0, o["state"].data_ptr() + 4 * w0, o["best"].data_ptr() + 8 * w0,
                                          o["gap"].data_ptr() + 8 * w0, o["margin"].data_ptr() + 8 * w0)
        rc = lib.dd_diploid_pairs_device(C.byref(db), C.c_void_p(self.t["hh"].data_ptr() + 8 * w0), C.c_void_p(self.t["ll"].data_ptr()),
                                         C.c_void_p(self.t["status"].data_ptr()) if status else None, C.c_void_p(self.t["prior"].data_ptr()),
                                         C.byref(res), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, capi.last_error()

    def results(self):
        torch.cuda.synchronize()
        r = {k: v.cpu().numpy() for k, v in self.out.items()}
        r["pair"] = r["pair"].reshape(self.W, 2)
        return r


@pytest.fixture(scope="module")
def resident():
    return Resident()


def assert_equal_to_twin(got, tw, windows=None):
    for k in capi.DIPLOID_PAIR_FIELDS:
        g, t = (got[k], tw[k]) if windows is None else (got[k][windows], tw[k][windows])
        if not same_bits(g, t):
            bad = np.flatnonzero([not same_bits(g[i], t[i]) for i in range(len(t))])
            raise AssertionError("%s differs at %d windows, first %d: %r against %r" % (k, len(bad), bad[0], g[bad[0]], t[bad[0]]))


def test_one_batch_of_more_windows_than_the_grid_has_workgroups(lib, resident):
    """Every synthetic window and every constructed case in one launch: 2,048 workgroups, one wavefront each, so the first windows' wavefronts
    take a second one; the windows of 65 and of DD_DIPPAIR_MAX_HAPS haplotypes (33 and 129 rounds of 64 pairs) among them."""
    c, tw = dc.build(), dc.twin()
    assert resident.W > GRID and 65 in c["nh"] and capi.DD_DIPPAIR_MAX_HAPS in c["nh"]
    resident.reset()
    resident.launch(lib)
    got = resident.results()
    assert_equal_to_twin(got, tw)
    assert set(got["state"].tolist()) == set(range(6))
    assert (got["state"][c["expect"] == dc.FUZZ] == capi.DD_DIPPAIR_CERTIFIED).all()
    for name, w in c["names"].items():
        assert got["state"][w] == c["expect"][w], name


def test_batches_of_one_window(lib, resident):
    """Each window as a launch of its own (one workgroup), on one stream; every output word of every window is written."""
    resident.reset()
    for w in range(resident.W):
        resident.launch(lib, w, 1)
    got = resident.results()
    assert_equal_to_twin(got, dc.twin())
    assert not (got["pair"] == FILL).any() and not (got["state"] == FILL).any() and not (got["best"] == -12345.5).any()


def test_a_part_of_the_batch_leaves_the_other_windows_alone_and_status_may_be_null(lib, resident):
    c, tw = dc.build(), dc.twin()
    w65 = int(np.flatnonzero(c["nh"] == 65)[0])
    resident.reset()
    resident.launch(lib, w65, 3)
    got = resident.results()
    inside = np.arange(w65, w65 + 3)
    assert_equal_to_twin(got, tw, inside)
    outside = np.setdiff1d(np.arange(resident.W), inside)
    assert (got["state"][outside] == FILL).all() and (got["pair"][outside] == FILL).all() and (got["gap"][outside] == -12345.5).all()
    resident.reset()
    resident.launch(lib, status=False)                                           # NULL status: every pair counts as computed
    got = resident.results()
    want = capi.diploid_pairs_host(c["ho"], c["ro"], c["ll"], c["prior"], None, nthreads=8)
    assert_equal_to_twin(got, want)
    assert got["state"][c["names"]["status"]] == capi.DD_DIPPAIR_CERTIFIED


# ---------------------------------------------------------------- chained in front of the realign launch
def chained(pb, hrp, prior, n_indels, ops_cap=8, tie_window=None, **kw):
    """launch(), the per-pair CIGARs, the pair launch and the realign launch that reads its `pair` on the device -> (results, pair outputs)."""
    dev = DeviceBatch(pb, capi.params_cli_defaults(), DEV, cigars=True, realign=True, ops_cap=ops_cap, hap_ref_pos=hrp, hap_n_indels=n_indels,
                      diploid_prior=prior, **kw)
    dev.launch()
    if tie_window is not None:                           # haplotype 1 of that window gets haplotype 0's likelihoods: with equal priors, a tie
        w = tie_window
        p0, R = int(pb.win_pair_off[w]), int(pb.a["win_read_off"][w + 1] - pb.a["win_read_off"][w])
        dev.out["ll"][p0 + R:p0 + 2 * R] = dev.out["ll"][p0:p0 + R].clone()
    for t in list(dev.cig.values()) + list(dev.rl.values()):
        t.fill_(FILL)
    dev.launch_cigars()
    dip = dev.launch_diploid_pairs()
    dev.launch_realign(capi.DD_REALIGN_PAIR, win_hap_pair=dip["pair"])
    return dev.results(), dev.diploid_pair_results()


def check_chain(pb, res, dp, prior, n_indels):
    """The pair outputs are the CPU evaluation's on the ll and status the launch left; the reads' rows follow from them."""
    want = capi.diploid_pairs_host(pb.a["win_hap_off"], pb.a["win_read_off"], res["ll"], prior, res["status"], nthreads=4)
    assert_equal_to_twin(dp, want)
    hap, none, pair = tgr.choose(pb, capi.DD_REALIGN_PAIR, res["ll"], None, dp["pair"].reshape(-1), n_indels)
    got = {k: res["realign_" + k] for k in ("hap", "status", "n_ops", "ops", "ref_off")}
    assert np.array_equal(got["hap"], hap)
    off = hap < 0
    assert np.array_equal(got["status"][off], none[off]) and (got["n_ops"][off] == 0).all() and (got["ref_off"][off] == -1).all()
    assert (got["ops"][off] == FILL).all()
    on = ~off
    for k in ("status", "n_ops", "ops", "ref_off"):                                # the row of the per-pair launch for the chosen pair
        assert np.array_equal(got[k][on], res["cigar_" + k][pair[on]]), k
    win = np.searchsorted(pb.a["win_read_off"], np.arange(pb.n_reads), side="right") - 1
    nh = np.diff(pb.a["win_hap_off"])[win]
    uncertified = dp["state"][win] != capi.DD_DIPPAIR_CERTIFIED
    assert (got["status"][uncertified & (nh > 0)] == capi.DD_REALIGN_BAD_PAIR).all()
    assert not (got["status"][~uncertified] == capi.DD_REALIGN_BAD_PAIR).any() and (got["hap"][~uncertified] >= 0).all()
    return got, uncertified


def window_priors(pb, seed, tie_window=None):
    rng = np.random.default_rng(seed)
    parts = []
    for w, H in enumerate(np.diff(pb.a["win_hap_off"])):
        p = -20.0 * rng.random((H, H))
        if w == tie_window:
            p[:] = -1e4
            p[:2, :2] = -1.5
        parts.append(p.reshape(-1))
    return np.concatenate(parts) if parts else np.zeros(0)


def test_chained_behind_the_main_launch_on_a_ragged_batch():
    pb = synth.generate_ragged(12, seed=2026, max_reads=90)
    hrp = cc.batch_hap_ref_pos(pb, 5)
    n_indels = np.random.default_rng(3).integers(0, 3, pb.n_haps).astype(np.int32)
    prior = window_priors(pb, 11, tie_window=4)
    res, dp = chained(pb, hrp, prior, n_indels, tie_window=4)
    got, uncertified = check_chain(pb, res, dp, prior, n_indels)
    assert dp["state"][4] == capi.DD_DIPPAIR_TIE and dp["gap"][4] == 0.0
    assert (np.delete(dp["state"], 4) == capi.DD_DIPPAIR_CERTIFIED).all()
    assert uncertified.sum() == pb.a["win_read_off"][5] - pb.a["win_read_off"][4]
    assert (got["status"] == capi.DD_CIGAR_OK).sum() > pb.n_reads // 2
    res1, dp1 = chained(pb, hrp, prior, n_indels, ops_cap=1, tie_window=4)       # the cap changes the rows, not the pairs
    assert_equal_to_twin(dp1, dp)
    check_chain(pb, res1, dp1, prior, n_indels)
    assert (res1["realign_status"] == capi.DD_CIGAR_OVERFLOW).any()


def test_chained_behind_the_long_window_launch():
    rng = np.random.default_rng(31)
    pbl = pack([tgr._long_window(rng, 900, 150), tgr._long_window(rng, 300, 1100, R=4), tgr._long_window(rng, 200, 100)])
    hrp = cc.batch_hap_ref_pos(pbl, 9)
    n_indels = np.array([0, 1] * 3, np.int32)
    prior = window_priors(pbl, 12)
    res, dp = chained(pbl, hrp, prior, n_indels, long_windows=True)
    check_chain(pbl, res, dp, prior, n_indels)
    assert (dp["state"] == capi.DD_DIPPAIR_CERTIFIED).all()
    res, dp = chained(pbl, hrp, prior, n_indels)                                  # without the option the long windows' pairs are not computed
    got, _ = check_chain(pbl, res, dp, prior, n_indels)
    assert list(dp["state"]) == [capi.DD_DIPPAIR_NOT_COMPUTED, capi.DD_DIPPAIR_NOT_COMPUTED, capi.DD_DIPPAIR_CERTIFIED]
    assert (got["status"][:10] == capi.DD_REALIGN_BAD_PAIR).all()


# ---------------------------------------------------------------- the host-pointer entry
def host_entry(lib, pb, hrp, prior, n_indels, ops_cap=8, options=0, with_hpos=False):
    from dindel_tgi_amd.batch import alloc_result
    p = capi.params_cli_defaults()
    arrs, res = alloc_result(pb)
    if not with_hpos:
        res.hpos = None
        arrs["hpos"][:] = -12345
    out, rl = capi.realign_arrays(pb.n_reads, ops_cap)
    pairs, dp = capi.diploid_pair_arrays(pb.n_windows)
    for v in list(out.values()) + [pairs["pair"], pairs["state"]]:
        v[...] = FILL
    b = pb.ctypes_batch()
    pr = np.ascontiguousarray(prior, np.float64)
    rc = lib.dd_compute_likelihoods_realign_diploid(C.byref(p), C.byref(b), C.byref(res), pr.ctypes.data_as(capi.c_f64p), n_indels.ctypes.data_as(capi.c_i32p),
                                                    hrp.ctypes.data_as(capi.c_i32p), None, C.byref(dp), C.byref(rl), ops_cap, 0, options)
    assert rc == 0, capi.last_error()
    return out, pairs, arrs


def assert_host_entry_matches(pb, out, pairs, arrs, res, dp):
    assert_equal_to_twin(pairs, dp)
    tgr.assert_same_reads(out, {k: res["realign_" + k] for k in ("hap", "status", "n_ops", "ops", "ref_off")})
    assert np.array_equal(arrs["ll"], res["ll"]) and np.array_equal(arrs["status"], res["status"])


def test_host_entry_with_and_without_alignments_and_with_long_windows(lib):
    pb = synth.generate_ragged(9, seed=515, max_reads=70)
    hrp = cc.batch_hap_ref_pos(pb, 6)
    n_indels = np.random.default_rng(8).integers(0, 3, pb.n_haps).astype(np.int32)
    prior = window_priors(pb, 13)
    res, dp = chained(pb, hrp, prior, n_indels)
    check_chain(pb, res, dp, prior, n_indels)
    out, pairs, arrs = host_entry(lib, pb, hrp, prior, n_indels)
    assert_host_entry_matches(pb, out, pairs, arrs, res, dp)
    assert (arrs["hpos"] == -12345).all() and (pairs["state"] == capi.DD_DIPPAIR_CERTIFIED).all()
    out2, pairs2, arrs2 = host_entry(lib, pb, hrp, prior, n_indels, with_hpos=True)      # asking for the alignments as well changes nothing else
    assert_host_entry_matches(pb, out2, pairs2, arrs2, res, dp)
    assert np.array_equal(arrs2["hpos"], res["hpos"])
    rng = np.random.default_rng(31)
    pbl = pack([tgr._long_window(rng, 900, 150), tgr._long_window(rng, 200, 100)])
    hrpl = cc.batch_hap_ref_pos(pbl, 9)
    nil, priorl = np.array([0, 1, 1, 0], np.int32), window_priors(pbl, 14)
    resl, dpl = chained(pbl, hrpl, priorl, nil, long_windows=True)
    outl, pairsl, arrsl = host_entry(lib, pbl, hrpl, priorl, nil, options=capi.DD_OPT_LONG_WINDOWS)
    assert_host_entry_matches(pbl, outl, pairsl, arrsl, resl, dpl)
    outn, pairsn, _ = host_entry(lib, pbl, hrpl, priorl, nil)                          # without the option the long window is not computed
    assert list(pairsn["state"]) == [capi.DD_DIPPAIR_NOT_COMPUTED, capi.DD_DIPPAIR_CERTIFIED] and (outn["status"][:6] == capi.DD_REALIGN_BAD_PAIR).all()


def test_host_entry_in_window_blocks(lib):
    """A batch of more than a million pairs runs as window blocks on two streams: each block's pair launch sits between its likelihood
    launches and its realign launch, and every block's windows and reads arrive, equal to the device-pointer chain's."""
    small = synth.generate(8, H=8, R=200, L=60, hap_len=100, seed=5)
    pb = synth.tile(small, 90)
    assert pb.n_pairs > 1100000
    hrp = cc.batch_hap_ref_pos(pb, 1)
    n_indels = np.random.default_rng(9).integers(0, 3, pb.n_haps).astype(np.int32)
    prior = window_priors(pb, 15)
    res, dp = chained(pb, hrp, prior, n_indels, ops_cap=4)
    want = capi.diploid_pairs_host(pb.a["win_hap_off"], pb.a["win_read_off"], res["ll"], prior, res["status"], nthreads=8)
    assert_equal_to_twin(dp, want)
    out, pairs, arrs = host_entry(lib, pb, hrp, prior, n_indels, ops_cap=4)
    assert_host_entry_matches(pb, out, pairs, arrs, res, dp)
    assert (pairs["state"] == capi.DD_DIPPAIR_CERTIFIED).sum() > pb.n_windows // 2
