"""The --faster kernels on the scenario batches of tests/_path_scenarios.py, bit-equal to the oracle (ddo_batch_fast).

dd_faster_long_kernel and dd_faster_kernel have one build each, but their LDS and tile layouts are functions of the batch's shape; the
adversarial families met them only through fuzz batches at a few shapes.

  dd_faster_long_kernel  the long batches (long_batch_for, many="items": more 16-pair items than the grid of the wide launch has
                         workgroups) at both ends of the haplotype range, the first length beyond dd_faster_kernel's and the last K
                         bound of the main model — through
                         dd_compute_likelihoods_faster_ex with and without the window of a 4,096-bp read, the device-pointer entry, and
                         page-locked result arrays inside guards
  dd_faster_kernel       batch_for at every point of the main grid, haplotypes of 30 .. 766 bp, with four, two and one pair areas per
                         wavefront (DD_FAST_GROUPS), and through DeviceBatch.launch_faster()

What a comparison leaves out is counted in tests/test_long_path_scenarios_cpu.py: the oracle's DD_PAIR_NAN and DD_PAIR_HAPSIZE pairs are compared
as statuses, the rejected window's pairs in the values the library defines (with_screened)."""
import ctypes as C
import time

import numpy as np
import pytest

from dindel_tgi_amd import capi
from tests import _oracle
from tests import _output_ownership as oo
from tests import _path_scenarios as ps
from tests._output_ownership import Guarded, alloc_poisoned, poisoned_arena
from tests.test_gpu_faster import assert_same_faster, run_faster
from tests.test_gpu_long_path_matrix import same_bytes

pytestmark = pytest.mark.gpu
FL = capi.DD_OPT_LONG_WINDOWS_FASTER
LONG_CASES = ps.FASTER_LONG_GRID
WALL = {}


@pytest.fixture(scope="module")
def lib():
    return capi.load()


def run_ex(lib, p, pb):
    """Poisoned arrays over a poisoned arena, as tests/test_gpu_faster.run_faster."""
    arrs, res = alloc_poisoned(pb)
    b = pb.ctypes_batch()
    with poisoned_arena():
        rc = lib.dd_compute_likelihoods_faster_ex(C.byref(p), C.byref(b), C.byref(res), 0, FL)
    assert rc == 0, capi.last_error()
    return arrs


def compare(got, want, pb, index, where):
    """assert_same_faster on the arrays of with_screened; a failure carries the leg, and the first differing pair's scenario family."""
    got, exp = ps.with_screened(got, want, pb, index)
    try:
        assert_same_faster(got, exp, pb)
    except AssertionError as e:
        ok = exp["status"][:pb.n_pairs] == capi.DD_PAIR_OK
        bad = [int(np.nonzero((got[k][:pb.n_pairs] != exp[k][:pb.n_pairs]) & (ok | (k == "status")))[0][:1].sum()) for k in ("status", "ll", "firstBase", "lastBase")
               if ((got[k][:pb.n_pairs] != exp[k][:pb.n_pairs]) & (ok | (k == "status"))).any()]
        raise AssertionError("%s: %s%s" % (where, e, "; first differing pair %d, family %s" % (min(bad), ps.family_of(min(bad), index)) if bad else ""))


def long_record(log, pb, p, where):
    cls, _mx, _n = capi.screen_windows_ex(p, pb, FL)
    pairs, items = ps.long_pairs(pb, cls)
    assert len(log) == 1, (where, log)
    assert log[0]["pairs"] == pairs and log[0]["ws_bytes"] <= capi.DD_FASTER_LONG_WS_BUDGET, (where, log[0], pairs)
    return log[0], items


@pytest.mark.parametrize("hl,L,mld", LONG_CASES, ids=["hap%d-L%d-mld%d" % c for c in LONG_CASES])
def test_every_path_on_the_faster_long_kernel(lib, hl, L, mld):
    import torch
    from dindel_tgi_amd.device import DeviceBatch
    t0 = time.time()
    tag = "dd_faster_long_kernel, haplotypes of %d bp, %d-bp reads, maxLengthDel %d" % (hl, L, mld)
    p = ps.params_for(mld, 1)                                                  # (this model has no mate prior: the mates are ordinary reads)
    wide, wide_index = ps.long_batch_for(hl, L, mld, wide=True, many="items")
    pb, index = ps.long_batch_for(hl, L, mld, wide=False, many="items")       # the wide batch without its last window: one oracle run for both
    want = _oracle.batch(p, wide, nthreads=16, faster=True)

    host = run_ex(lib, p, pb)
    assert lib.dd_last_direct_outputs() == 0
    rec, items = long_record(capi.faster_long_launch_log(), pb, p, tag + ", host call")
    compare(host, want, pb, index, tag + ", host call")
    assert rec["max_pairs_per_wg"] >= 16, (rec, items)

    got = run_ex(lib, p, wide)
    wrec, witems = long_record(capi.faster_long_launch_log(), wide, p, tag + ", wide")
    compare(got, want, wide, wide_index, tag + ", wide")
    assert wrec["max_read"] == ps.LONG_WIDE_LEN and witems > wrec["grid"] and wrec["max_items_per_wg"] >= 2 and wrec["max_pairs_per_wg"] > 16, (wrec, witems)
    print("faster long matrix hap %d: grid %d items %d max_items_per_wg %d; wide: grid %d items %d max_items_per_wg %d"
          % (hl, rec["grid"], items, rec["max_items_per_wg"], wrec["grid"], witems, wrec["max_items_per_wg"]))

    g = Guarded(lib, pb)
    try:
        b = pb.ctypes_batch()
        rc = lib.dd_compute_likelihoods_faster_ex(C.byref(p), C.byref(b), C.byref(g.res), 0, FL)
        assert rc == 0, capi.last_error()
        assert lib.dd_last_direct_outputs() >= 10, lib.dd_last_direct_outputs()
        left = g.check(host, pb, index, tag + ", guarded")
        print("faster long matrix hap %d: body sentinels left where the library does not write: %r" % (hl, left))
        compare({k: g.body(k).copy() for k, _t in capi.RESULT_FIELDS}, want, pb, index, tag + ", guarded")
    finally:
        g.release()

    dev = DeviceBatch(pb, p, "cuda:0", long_windows_faster=True)
    assert dev.n_long == pb.n_windows - 3
    dev.launch_faster()
    torch.cuda.synchronize()
    long_record(capi.faster_long_launch_log(), pb, p, tag + ", device")
    res = dev.results()
    compare(res, want, pb, index, tag + ", device")
    same_bytes(res, host, pb, index, tag + ", device")
    del dev
    WALL[("long", hl, L, mld)] = time.time() - t0
    print("faster long matrix haplotypes %d L %d mld %d: %.1f s" % (hl, L, mld, WALL[("long", hl, L, mld)]))


@pytest.mark.parametrize("mld,L", ps.GRID, ids=["mld%d-L%d" % c for c in ps.GRID])
def test_every_path_on_the_faster_kernel(lib, monkeypatch, mld, L):
    import torch
    from dindel_tgi_amd.device import DeviceBatch
    t0 = time.time()
    p = ps.params_for(mld, 1)
    seen = set()
    for hl in ps.FASTER_HAP_LENGTHS:
        if hl not in ps.hap_lengths(mld):
            continue
        pb, index = ps.batch_for(hl, L, mld)
        want = _oracle.batch(p, pb, nthreads=16, faster=True)
        own = oo.must_write(pb, want, index, faster=True)    # every call below starts from poisoned buffers: what it must write, and nothing else
        tag = "dd_faster_kernel, maxLengthDel %d, %d-bp reads, haplotypes of %d bp" % (mld, L, hl)
        host = None
        for groups in (None, "2", "1"):
            if groups is None:
                monkeypatch.delenv("DD_FAST_GROUPS", raising=False)
            else:
                monkeypatch.setenv("DD_FAST_GROUPS", groups)
            got = run_faster(lib, p, pb)
            ll = np.zeros(8, np.int32)
            lib.dd_last_launch(C.byref((C.c_int32 * 8).from_buffer(ll)))
            assert int(ll[0]) == (int(groups) if groups else 4), (tag, groups, ll)     # four pair areas fit at every shape within DD_MAX_*
            seen.add(int(ll[0]))
            compare(got, want, pb, index, tag + ", %s pair areas per wavefront" % (groups or "4"))
            oo.assert_owned(got, want, pb, own, tag + ", %s pair areas per wavefront" % (groups or "4"))
            host = host or got
        monkeypatch.delenv("DD_FAST_GROUPS", raising=False)
        dev = DeviceBatch(pb, p, "cuda:0")
        assert dev.n_skipped == 1
        guarded = oo.GuardedDevice(dev)                      # its result tensors: poison inside 256-byte guards
        dev.launch_faster()
        torch.cuda.synchronize()
        res = dev.results()
        compare(res, want, pb, index, tag + ", device-pointer path")
        same_bytes(res, host, pb, index, tag + ", device-pointer path")
        oo.assert_owned(res, want, pb, own, tag + ", device-pointer path")
        guarded.check(tag + ", device-pointer path")
        del guarded, dev
    assert seen == {1, 2, 4}
    WALL[("main", mld, L)] = time.time() - t0
    print("faster matrix mld %d L %d: %.1f s" % (mld, L, WALL[("main", mld, L)]))
