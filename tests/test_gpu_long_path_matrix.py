"""Every per-pair code path on every build of dd_long_kernel<K> (K = 1, 2, 4, 8, 16), later items of a workgroup included, bit-equal to the
oracle.

tests/test_gpu_long_windows.py runs each per-pair path on one K and a persistent round on K = 4 only; a compiler fault is per build, and it
showed on the later items of a persistent workgroup.  Here the scenario batch of tests/_path_scenarios.py, forced onto the long
path by one 1,025-bp read per window (long_batch_for; tests/test_long_path_scenarios_cpu.py shows on the oracle what it reaches), goes
through every K at haplotype lengths on both sides of every K bound, with more pairs than the persistent grid has workgroups.  Legs per
case, all against one oracle run:

  host      dd_compute_likelihoods_ex into pageable arrays: one long launch of the expected K over the long windows' pairs
  wide      the same with one window of a 4,096-bp read appended: the workspace budget shrinks the grid, workgroups take several pairs
  guarded   the host call with every result array page-locked (written in place), inside 256-byte guards on both sides
  device    DeviceBatch(long_windows=True).launch(): byte-equal to the host call
  unmapped  mapUnmappedReads = 0 on the same arrays: only the mates window's pairs change

A failure names K, the leg, the scenario family and the pair."""
import ctypes as C
import time

import numpy as np
import pytest

from dindel_tgi_amd import capi
from dindel_tgi_amd.batch import result_lengths
from tests import _oracle
from tests import _path_scenarios as ps
from tests._output_ownership import PER_ELEMENT, Guarded, alloc_poisoned, poisoned_arena
from tests.test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

CASES = ps.LONG_GRID
IDS = ["hap%d-L%d-mld%d-K%d" % c for c in CASES]

RECORDS = {}             # K -> launch records of the module's long launches
SHORT_ON = set()         # K on which a computed haplotype shorter than 128 K bp ran
RAN, WALL = set(), {}


@pytest.fixture(scope="module")
def lib():
    return capi.load()


def run_ex(lib, p, pb):
    """Poisoned arrays over a poisoned arena, as tests/test_gpu_parity.run_host_api."""
    arrs, res = alloc_poisoned(pb)
    b = pb.ctypes_batch()
    with poisoned_arena():
        rc = lib.dd_compute_likelihoods_ex(C.byref(p), C.byref(b), C.byref(res), 0, capi.DD_OPT_LONG_WINDOWS)
    assert rc == 0, capi.last_error()
    return arrs


def compare(got, want, pb, index, where):
    """Bit equality with the oracle (tests/test_gpu_parity.assert_same and the hpos of every computed pair); a difference is reported with
    the leg, the pair's scenario family, its index and its shape."""
    got, exp = ps.with_screened(got, want, pb, index)
    diff = ps.first_difference(got, exp, pb, index)
    if diff is not None:
        key, elem, pair, family = diff
        w = int(np.searchsorted(pb.win_pair_off, pair, side="right")) - 1
        R = int(pb.a["win_read_off"][w + 1] - pb.a["win_read_off"][w])
        h, r = divmod(pair - int(pb.win_pair_off[w]), R)
        g, q = int(pb.a["win_hap_off"][w]) + h, int(pb.a["win_read_off"][w]) + r
        raise AssertionError("%s: family %s, pair %d (window %d, %d-bp haplotype x %d-bp read): %s[%d] is %r, the oracle has %r"
                             % (where, family, pair, w, int(pb.a["hap_seq_off"][g + 1] - pb.a["hap_seq_off"][g]),
                                int(pb.a["read_seq_off"][q + 1] - pb.a["read_seq_off"][q]), key, elem, got[key][elem], exp[key][elem]))
    assert_same(got, exp, pb)


def long_record(log, pb, p, K, where, options=capi.DD_OPT_LONG_WINDOWS):
    """The one long launch of the last call: the expected K over exactly the long windows' pairs."""
    cls, _mx, _n = capi.screen_windows_ex(p, pb, options)
    pairs, _items = ps.long_pairs(pb, cls)
    assert len(log) == 1, (where, log)
    assert log[0]["K"] == K and log[0]["pairs"] == pairs and log[0]["ws_bytes"] <= capi.DD_LONG_WS_BUDGET, (where, log[0], pairs)
    return log[0]


def same_bytes(got, host, pb, index, where):
    """got byte-equal to host in every result array, but for what the library does not write (with_screened: the rejected window's other
    values; of a pair that failed — hapSize error, or DD_PAIR_NAN in the --faster model — everything but its status and coverage flags, as in
    assert_same and assert_same_faster)."""
    a, b = ps.with_screened(got, host, pb, index)
    failed = np.isin(host["status"][:pb.n_pairs], (capi.DD_PAIR_HAPSIZE, capi.DD_PAIR_NAN))
    skip = np.isin(ps.element_pairs(pb)["hpos"][:pb.hpos_len], np.nonzero(failed)[0])
    n = result_lengths(pb)
    for k, _typ in capi.RESULT_FIELDS:
        x, y = a[k][:n[k]], b[k][:n[k]]
        if k == "hpos":
            x, y = x[~skip], y[~skip]
        elif k not in PER_ELEMENT and k != "status":
            x, y = x[~failed], y[~failed]
        assert x.tobytes() == y.tobytes(), "%s: %s differs from the host call at element %d" % (where, k, int(np.nonzero(x != y)[0][0]))


def spliced(want, off, pb, w):
    """want with window w's results replaced by those of `off` (an oracle run of that window alone)."""
    out = {k: v.copy() for k, v in want.items()}
    for k, o in (("hpos", pb.win_hpos_off), ("var_covered", pb.win_varcov_off), ("var_fcov", pb.win_varcov_off), ("onHap", pb.a["win_read_off"])):
        out[k][int(o[w]):int(o[w + 1])] = off[k][int(o[w]):int(o[w + 1])]
    for k in out:
        if k not in PER_ELEMENT:
            out[k][int(pb.win_pair_off[w]):int(pb.win_pair_off[w + 1])] = off[k][int(pb.win_pair_off[w]):int(pb.win_pair_off[w + 1])]
    return out


@pytest.mark.parametrize("hl,L,mld,K", CASES, ids=IDS)
def test_every_path_on_every_long_build(lib, hl, L, mld, K):
    import torch
    from dindel_tgi_amd.device import DeviceBatch
    t0 = time.time()
    tag = "dd_long_kernel<%d>, haplotypes of %d bp, %d-bp reads, maxLengthDel %d" % (K, hl, L, mld)
    p = ps.params_for(mld, 1)
    wide, wide_index = ps.long_batch_for(hl, L, mld, wide=True, many=True)
    pb, index = ps.long_batch_for(hl, L, mld, wide=False, many=True)          # the wide batch without its last window: one oracle run for both
    want = _oracle.batch(p, wide, nthreads=16)

    # host: pageable results
    host = run_ex(lib, p, pb)
    assert lib.dd_last_direct_outputs() == 0
    rec = long_record(capi.long_launch_log(), pb, p, K, tag + ", host call")
    RECORDS.setdefault(K, []).append(rec)
    compare(host, want, pb, index, tag + ", host call")
    assert rec["pairs"] > 2 * rec["grid"] and rec["max_pairs_per_wg"] >= 3, rec          # (the builder sizes long.many for that)
    hs_win = int(np.searchsorted(pb.win_pair_off, index["screened.hapsize"][0], side="right")) - 1
    small_pairs = np.arange(int(pb.win_pair_off[hs_win]), int(index["screened.hapsize"][0]))     # the hapSize window's 80-bp haplotype
    if (host["status"][small_pairs] == capi.DD_PAIR_OK).all() and min(80, hl) < 128 * K:
        SHORT_ON.add(K)

    # wide: a 4,096-bp read shrinks the grid to what the workspace budget holds
    got = run_ex(lib, p, wide)
    wrec = long_record(capi.long_launch_log(), wide, p, K, tag + ", wide")
    RECORDS[K].append(wrec)
    compare(got, want, wide, wide_index, tag + ", wide")
    assert wrec["max_read"] == ps.LONG_WIDE_LEN and wrec["grid"] <= ps.long_grid_bound(hl, ps.LONG_WIDE_LEN)[1], wrec
    assert wrec["pairs"] > wrec["grid"] and wrec["max_pairs_per_wg"] >= 2, wrec
    print("long matrix K %d hap %d: grid %d pairs %d max_pairs_per_wg %d; wide: grid %d pairs %d max_pairs_per_wg %d"
          % (K, hl, rec["grid"], rec["pairs"], rec["max_pairs_per_wg"], wrec["grid"], wrec["pairs"], wrec["max_pairs_per_wg"]))

    # guarded: page-locked arrays written in place, interior pointers
    g = Guarded(lib, pb)
    try:
        b = pb.ctypes_batch()
        rc = lib.dd_compute_likelihoods_ex(C.byref(p), C.byref(b), C.byref(g.res), 0, capi.DD_OPT_LONG_WINDOWS)
        assert rc == 0, capi.last_error()
        assert lib.dd_last_direct_outputs() >= 10, lib.dd_last_direct_outputs()
        long_record(capi.long_launch_log(), pb, p, K, tag + ", guarded")
        left = g.check(host, pb, index, tag + ", guarded")
        print("long matrix K %d hap %d: body sentinels left where the library does not write: %r" % (K, hl, left))
        compare({k: g.body(k).copy() for k, _t in capi.RESULT_FIELDS}, want, pb, index, tag + ", guarded")
    finally:
        g.release()

    # device: the device-pointer entry
    dev = DeviceBatch(pb, p, "cuda:0", long_windows=True)
    assert dev.n_long == pb.n_windows - 3
    dev.launch()
    torch.cuda.synchronize()
    long_record(capi.long_launch_log(), pb, p, K, tag + ", device")
    res = dev.results()
    compare(res, want, pb, index, tag + ", device")
    same_bytes(res, host, pb, index, tag + ", device")
    del dev

    # unmapped: the mate prior switched off moves the mates window's pairs only
    p0 = ps.params_for(mld, 0)
    w = int(index["mates.window"][0])
    want0 = spliced(want, _oracle.batch(p0, pb, first_window=w, n_win=1), pb, w)
    got = run_ex(lib, p0, pb)
    long_record(capi.long_launch_log(), pb, p0, K, tag + ", mapUnmappedReads 0")
    compare(got, want0, pb, index, tag + ", mapUnmappedReads 0")
    assert (got["ll"][index["mates.usable"]] != host["ll"][index["mates.usable"]]).any()
    outside = np.ones(pb.n_pairs, bool)
    outside[int(pb.win_pair_off[w]):int(pb.win_pair_off[w + 1])] = False
    assert got["ll"][:pb.n_pairs][outside].tobytes() == host["ll"][:pb.n_pairs][outside].tobytes()

    RAN.add((hl, L, mld, K))
    WALL[(hl, L, mld, K)] = time.time() - t0
    print("long matrix K %d haplotypes %d L %d mld %d: %.1f s" % (K, hl, L, mld, WALL[(hl, L, mld, K)]))


def test_the_matrix_launched_every_long_build_with_later_items(lib):
    """From the launch records the cases above collected: all five K ran, each with a launch in which some workgroup took two pairs or more,
    and a computed haplotype shorter than 128 K bp (most of the workgroup's states are padding) ran on every K >= 2."""
    if RAN != set(CASES):
        pytest.skip("needs every case of test_every_path_on_every_long_build in the same run (%d of %d ran)" % (len(RAN), len(CASES)))
    print("long matrix wall time per case: " + ", ".join("hap%d-L%d-mld%d-K%d %.1f s" % (k + (v,)) for k, v in sorted(WALL.items())))
    for K, recs in sorted(RECORDS.items()):
        print("long matrix K %d: " % K + "; ".join("grid %d pairs %d max_pairs_per_wg %d" % (r["grid"], r["pairs"], r["max_pairs_per_wg"]) for r in recs))
    assert set(RECORDS) == {1, 2, 4, 8, 16}, sorted(RECORDS)
    assert all(any(r["max_pairs_per_wg"] >= 2 for r in recs) for recs in RECORDS.values())
    assert SHORT_ON >= {2, 4, 8, 16}, sorted(SHORT_ON)
