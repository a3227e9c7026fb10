"""GPU: the device-side getCIGAR (dd_cigars_device, cigar_kernel.hip) against the host specification, dindel::getCIGAR through
ddh_get_cigar, on the same arrays: operations, their count, the reference offset and the status / throw of every pair.  Exact equality.

The kernel takes hpos as an input, so the tests feed it (a) what the likelihood kernels wrote and (b) generated alignments that reach every
branch of host/cigar.cpp (tests/_cigar_cases.py; tests/test_cigars_cpu.py checks that reach on the CPU).  Output arrays start out filled
with a pattern, so a word the kernel must not write is seen if it does."""
import ctypes as C

import numpy as np
import pytest
import torch

from dindel_tgi_amd import capi, synth
from dindel_tgi_amd.batch import ReadRec, Window, alloc_result, alloc_result_pinned, pack, result_lengths
from dindel_tgi_amd.device import DeviceBatch
from tests import _cigar_cases as cc

pytestmark = pytest.mark.gpu
FILL = 0x3B3B3B3B


def device_cigars(pb, hap_ref_pos, hap_aligned=None, ops_cap=8, hpos=None, status=None, launch="main", **kw):
    """DeviceBatch(cigars=True): the likelihood launch (or the given hpos / status instead), then launch_cigars -> (results, hpos, status)."""
    dev = DeviceBatch(pb, capi.params_cli_defaults(), "cuda:0", cigars=True, ops_cap=ops_cap, hap_ref_pos=hap_ref_pos, hap_aligned=hap_aligned, **kw)
    if launch == "main":
        dev.launch()
    elif launch == "faster":
        dev.launch_faster()
    if hpos is not None:
        dev.out["hpos"][:len(hpos)] = torch.from_numpy(np.ascontiguousarray(hpos, np.int16)).to(dev.device)
    if status is not None:
        dev.out["status"][:len(status)] = torch.from_numpy(np.ascontiguousarray(status, np.int32)).to(dev.device)
    for t in dev.cig.values():
        t.fill_(FILL)
    dev.launch_cigars()
    res = dev.results()
    got = {k: res["cigar_" + k] for k in ("n_ops", "ops", "ref_off", "status")}
    return got, res["hpos"], res["status"]


def check(pb, hap_ref_pos, hap_aligned=None, ops_cap=8, **kw):
    got, hpos, status = device_cigars(pb, hap_ref_pos, hap_aligned, ops_cap, **kw)
    want, outcomes = cc.expected(pb, hpos, hap_ref_pos, hap_aligned, status, ops_cap, FILL)
    cc.assert_equal(got, want, outcomes)
    return got, want, outcomes


def some_unaligned(pb, seed):
    hal = np.ones(pb.n_haps, np.uint8)
    hal[np.random.default_rng(seed).random(pb.n_haps) < 0.15] = 0
    hal[0] = 0
    return hal


@pytest.mark.parametrize("cfg", [dict(n=6, H=4, R=40, L=36, hap_len=120), dict(n=5, H=5, R=60, L=100, hap_len=130, vary_read_len=True, mixed_quals=True),
                                 dict(n=4, H=4, R=30, L=150, hap_len=140, max_indel=5), dict(n=3, H=3, R=24, L=300, hap_len=260, vary_read_len=True),
                                 dict(n=2, H=3, R=12, L=1024, hap_len=700, max_indel=5)])
def test_hpos_of_the_likelihood_kernels(cfg):
    """(a) seeded batches with indels, reads of 36..1,024 bp (two and more 64-base chunks, ragged tails), haplotypes whose refHpos has
    deletions and insertions against the reference, some haplotypes not aligned."""
    cfg = dict(cfg)
    pb = synth.generate(cfg.pop("n"), seed=1234 + cfg["L"], **cfg)
    hrp = cc.batch_hap_ref_pos(pb, 77)
    got, want, _ = check(pb, hrp, some_unaligned(pb, 3))
    done = (want["status"] == capi.DD_CIGAR_OK) | (want["status"] == capi.DD_CIGAR_OVERFLOW)   # (a 1,024-bp read crosses more than 8 events)
    assert done.sum() > pb.n_pairs // 2 and (want["status"] == capi.DD_CIGAR_HAP_NOT_ALIGNED).any()
    assert (want["n_ops"] >= 3).any()                                    # indels against the reference are there


def test_hpos_of_a_ragged_batch():
    pb = synth.generate_ragged(14, seed=99, max_reads=120)
    check(pb, cc.batch_hap_ref_pos(pb, 5), some_unaligned(pb, 8))


def test_adversarial_alignments_reach_every_branch_and_throw():
    """(b) sequences no traceback emits: every branch, the fall-through and every throw the walk can reach; single-base and all-negative
    reads; events on bases 63 / 64 / 65."""
    pb, hpos, hrp = cc.adversarial_batch()
    assert cc.coverage(pb, hpos, hrp) == cc.BRANCHES                     # on the CPU, before the launch
    got, want, outcomes = check(pb, hrp, hpos=hpos, launch=None, ops_cap=16)
    assert {o for o in outcomes if isinstance(o, int)} == {-4, -5, -6, -7}
    assert set(np.unique(want["status"])) >= {capi.DD_CIGAR_OK, capi.DD_CIGAR_ERROR2, capi.DD_CIGAR_ERROR3, capi.DD_CIGAR_ERROR4, capi.DD_CIGAR_IMPOSSIBLE}


def test_overflow_reports_the_true_count_and_the_first_operations():
    """(c) ops_cap = 2."""
    pb, hpos, hrp = cc.adversarial_batch()
    got, want, _ = check(pb, hrp, hpos=hpos, launch=None, ops_cap=2)
    over = want["status"] == capi.DD_CIGAR_OVERFLOW
    assert over.sum() > 50 and (got["n_ops"][over] > 2).all() and (got["ops"][over] != FILL).all()
    check(pb, hrp, hpos=hpos, launch=None, ops_cap=1)


def test_pairs_without_likelihood_are_marked_and_left_alone():
    """(d) a non-zero dd_result.status: DD_CIGAR_NOT_COMPUTED, no operation written, hpos (out of range here) not read."""
    pb, hpos, hrp = cc.adversarial_batch()
    rng = np.random.default_rng(2)
    status = rng.choice([0, 0, 0, capi.DD_PAIR_HAPSIZE, capi.DD_PAIR_NAN, capi.DD_PAIR_LLPOS, capi.DD_PAIR_UNSUPPORTED], pb.n_pairs).astype(np.int32)
    hpos = hpos.copy()
    for p, _g, sl in cc.pair_hpos_slices(pb):
        if status[p]:
            hpos[sl] = 32000
    got, want, _ = check(pb, hrp, hpos=hpos, status=status, launch=None)
    skipped = status != 0
    assert (got["status"][skipped] == capi.DD_CIGAR_NOT_COMPUTED).all() and (got["ops"][skipped] == FILL).all()


def _long_window(rng, hap_len, L, R=6):
    hap = "".join(rng.choice(list("ACGT"), hap_len))
    hap2 = hap[:hap_len // 2] + "GT" + hap[hap_len // 2:]
    reads = []
    for _ in range(R):
        off = int(rng.integers(-L // 3, max(1, hap_len - L // 2)))
        src = hap2 if rng.random() < 0.5 else hap
        seq = "".join(src[i] if 0 <= i < len(src) else "A" for i in range(off, off + L))
        reads.append(ReadRec(seq, [0.999] * L, 0.9999, 1000 + off))
    return Window(1000, [hap, hap2], reads)


def test_after_the_long_window_and_faster_launches():
    """(e) the CIGAR launch only reads hpos: behind dd_launch_device_long, dd_launch_device_faster and dd_launch_device_faster_long it gives
    what the host gives on the hpos those kernels wrote."""
    rng = np.random.default_rng(31)
    pb = pack([_long_window(rng, 900, 150), _long_window(rng, 300, 1100, R=4), _long_window(rng, 200, 100)])
    hrp = cc.batch_hap_ref_pos(pb, 9)
    got, want, _ = check(pb, hrp, long_windows=True)
    assert np.isin(want["status"], [capi.DD_CIGAR_OK, capi.DD_CIGAR_OVERFLOW]).all()   # the long windows were computed, so their CIGARs are
    got, want, _ = check(pb, hrp)                                        # without the option the long windows' pairs are not computed
    assert (want["status"] == capi.DD_CIGAR_NOT_COMPUTED).sum() == 2 * 6 + 2 * 4
    check(pb, hrp, launch="faster", long_windows_faster=True)
    pb2 = synth.generate(4, H=4, R=40, L=100, hap_len=120, seed=8)
    check(pb2, cc.batch_hap_ref_pos(pb2, 2), some_unaligned(pb2, 1), launch="faster")


def test_more_pairs_than_one_round_of_the_grid():
    """(f) the grid is persistent (2,048 workgroups x 4 wavefronts): 3 rounds and a partial one."""
    rng = np.random.default_rng(6)
    pb = cc.csr_batch([([200, 200, 200], [int(rng.integers(1, 90)) for _ in range(230)]) for _ in range(40)])
    assert pb.n_pairs > 3 * 2048 * 4
    hrp = cc.batch_hap_ref_pos(pb, 4)
    hpos = np.zeros(pb.hpos_len, np.int16)
    for _p, _g, sl in cc.pair_hpos_slices(pb):
        L = sl.stop - sl.start
        start = int(rng.integers(-5, 120))
        v = np.arange(start, start + L)
        k = int(rng.integers(2, L - 3)) if L > 8 and rng.random() < 0.5 else -1
        ins = k >= 0 and rng.random() < 0.5
        if k >= 0 and not ins:
            v[k:] += int(rng.integers(1, 4))                             # deletion
        if ins:
            v[k + 1:] -= 1                                               # insertion of base k
        v = np.where(v < 0, capi.DD_HPOS_LO, np.where(v >= 200, capi.DD_HPOS_RO, v))
        if ins and 0 <= v[k - 1]:
            v[k] = capi.DD_HPOS_INS_KEY0 - int(v[k - 1]) - 1
        hpos[sl] = v
    check(pb, hrp, hpos=hpos, launch=None)


def host_entry(lib, pb, hrp, hal, ops_cap=8, options=0, with_hpos=False, result=None):
    p = capi.params_cli_defaults()
    arrs, res = result or alloc_result(pb)
    if not with_hpos:
        res.hpos = None
        arrs["hpos"][:] = -12345
    n = pb.n_pairs
    out = dict(n_ops=np.full(n, FILL, np.int32), ops=np.full((n, ops_cap), FILL, np.uint32), ref_off=np.full(n, FILL, np.int32),
               status=np.full(n, FILL, np.int32))
    cig = capi.dd_cigar_result(*[out[k].ctypes.data for k in ("n_ops", "ops", "ref_off", "status")])
    b = pb.ctypes_batch()
    rc = lib.dd_compute_likelihoods_cigars(C.byref(p), C.byref(b), C.byref(res), hrp.ctypes.data_as(capi.c_i32p),
                                           None if hal is None else hal.ctypes.data_as(capi.c_u8p), C.byref(cig), ops_cap, 0, options)
    assert rc == 0, capi.last_error()
    return out, arrs


def test_host_entry_keeps_the_alignments_on_the_device(lib):
    """dd_compute_likelihoods_cigars with r->hpos == NULL: the CIGARs of the device-pointer path, the other outputs of dd_compute_likelihoods,
    and no alignment copied back.  A pair's operation slots beyond its count come back as zero on this path."""
    pb = synth.generate(5, H=5, R=60, L=100, hap_len=130, seed=1334, vary_read_len=True, mixed_quals=True)
    hrp, hal = cc.batch_hap_ref_pos(pb, 77), some_unaligned(pb, 3)
    ref, hpos, status = device_cigars(pb, hrp, hal)
    want, outcomes = cc.expected(pb, hpos, hrp, hal, status, 8, 0)
    got, arrs = host_entry(lib, pb, hrp, hal)
    cc.assert_equal(got, want, outcomes)
    assert (arrs["hpos"] == -12345).all()
    plain, _res = alloc_result(pb)
    p = capi.params_cli_defaults()
    b = pb.ctypes_batch()
    assert lib.dd_compute_likelihoods(C.byref(p), C.byref(b), C.byref(_res), 0) == 0
    for k in plain:
        if k != "hpos":
            assert np.array_equal(plain[k], arrs[k]), k
    got2, arrs2 = host_entry(lib, pb, hrp, hal, with_hpos=True)          # asking for the alignments as well changes nothing else
    cc.assert_equal(got2, want, outcomes)
    assert np.array_equal(arrs2["hpos"], plain["hpos"])
    # with the long-window option
    rng = np.random.default_rng(31)
    pbl = pack([_long_window(rng, 900, 150), _long_window(rng, 200, 100)])
    hrpl = cc.batch_hap_ref_pos(pbl, 9)
    _ref, hposl, statusl = device_cigars(pbl, hrpl, long_windows=True)
    wantl, outl = cc.expected(pbl, hposl, hrpl, None, statusl, 8, 0)
    gotl, _ = host_entry(lib, pbl, hrpl, None, options=capi.DD_OPT_LONG_WINDOWS)
    cc.assert_equal(gotl, wantl, outl)


def with_page_locked_results(lib, pb, entry):
    """entry(result) with every dd_result array from dd_host_alloc (allocated as tests/test_gpu_parity.py::test_pinned_outputs_are_written_in_place
    does) -> (what the entry filled besides, copies of the dd_result arrays, how many of them the entry let the kernels write in place, how many
    a plain dd_compute_likelihoods call does on the same memory)."""
    arrs, res, release = alloc_result_pinned(pb)
    try:
        p, b = capi.params_cli_defaults(), pb.ctypes_batch()
        assert lib.dd_compute_likelihoods(C.byref(p), C.byref(b), C.byref(res), 0) == 0, capi.last_error()
        plain = lib.dd_last_direct_outputs()
        assert plain >= 10
        for a in arrs.values():
            a.view(np.uint8)[...] = 0x55
        out, _ = entry((arrs, res))
        return out, {k: a.copy() for k, a in arrs.items()}, lib.dd_last_direct_outputs(), plain
    finally:
        release()


def assert_same_bytes(pb, pageable, pinned):
    for k, n in result_lengths(pb).items():
        assert np.array_equal(pageable[k][:n].view(np.uint8), pinned[k][:n].view(np.uint8)), k


def test_host_entry_with_page_locked_results(lib):
    """dd_compute_likelihoods_cigars with every dd_result array in page-locked memory: the CIGAR launch reads hpos on the device, so hpos — which
    a plain call lets the kernels write in place — is staged in HBM and copied back; every byte equals the pageable call's."""
    pb = synth.generate(5, H=5, R=60, L=100, hap_len=130, seed=1334, vary_read_len=True, mixed_quals=True)
    hrp, hal = cc.batch_hap_ref_pos(pb, 77), some_unaligned(pb, 3)
    want, pageable = host_entry(lib, pb, hrp, hal, with_hpos=True)
    assert lib.dd_last_direct_outputs() == 0
    got, pinned, direct, plain = with_page_locked_results(lib, pb, lambda result: host_entry(lib, pb, hrp, hal, with_hpos=True, result=result))
    assert direct == plain - 1
    assert_same_bytes(pb, pageable, pinned)
    for k in want:
        assert np.array_equal(want[k], got[k]), k


def test_host_entry_in_window_blocks(lib):
    """A batch of more than a million pairs runs as window blocks on two streams: every block's CIGARs arrive, equal to the
    device-pointer path's."""
    small = synth.generate(8, H=8, R=200, L=60, hap_len=100, seed=5)
    pb = synth.tile(small, 90)
    assert pb.n_pairs > 1100000
    hrp = cc.batch_hap_ref_pos(pb, 1)
    ref, _hpos, _status = device_cigars(pb, hrp, ops_cap=4)
    assert (ref["status"] == capi.DD_CIGAR_OK).any() and (ref["status"] != capi.DD_CIGAR_NOT_COMPUTED).all()
    got, _ = host_entry(lib, pb, hrp, None, ops_cap=4)
    for k in ("status", "n_ops", "ref_off"):
        assert np.array_equal(got[k], ref[k]), k
    written = np.arange(4)[None, :] < np.minimum(ref["n_ops"], 4)[:, None]
    finished = np.isin(ref["status"], [capi.DD_CIGAR_OK, capi.DD_CIGAR_OVERFLOW])[:, None]    # (a pair that threw may have written operations before)
    assert np.array_equal(got["ops"][written], ref["ops"][written]) and (got["ops"][~written & finished] == 0).all()
    # the first window against the host specification
    sl = slice(0, int(small.win_pair_off[1]))
    want, outcomes = cc.expected(small.slice_windows(0, 1), _hpos[:int(small.win_hpos_off[1])], hrp[:int(small.a["hap_seq_off"][8])], None,
                                 _status[sl], 4, 0)
    for k in ("status", "n_ops", "ref_off"):
        assert np.array_equal(got[k][sl], want[k]), k
