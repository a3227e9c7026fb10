"""GPU: the --faster model's indel-map key count on the device (dd_indel_keys_device, indel_keys_kernel.hip) against the CPU evaluation of
the same header (dd_indel_keys_host) on the same arrays, every pair, exact equality.

The kernel takes hpos as an input, so the tests feed it (a) what the --faster kernels wrote and (b) alignments no traceback emits
(tests/_indel_keys_cases.py; tests/test_indel_keys_cpu.py checks the CPU evaluation against a Python restatement and against the adapter's
own walk).  The output starts out filled with a pattern, so a pair the kernel does not write is seen."""
import ctypes as C

import numpy as np
import pytest
import torch

from dindel_tgi_amd import capi, synth
from dindel_tgi_amd.batch import ReadRec, Window, alloc_result, pack
from dindel_tgi_amd.device import DeviceBatch
from tests import _cigar_cases as cc
from tests import _indel_keys_cases as ik

pytestmark = pytest.mark.gpu
FILL = 0x3B3B


def device_keys(pb, hpos=None, status=None, launch="faster", stream=None, **kw):
    """DeviceBatch(indel_keys=True): the --faster launch (or the given hpos / status instead), then launch_indel_keys ->
    (keys, hpos, status, dev)."""
    dev = DeviceBatch(pb, capi.params_cli_defaults(), "cuda:0", indel_keys=True, **kw)
    if launch == "faster":
        dev.launch_faster()
    if hpos is not None:
        dev.out["hpos"][:len(hpos)] = torch.from_numpy(np.ascontiguousarray(hpos, np.int16)).to(dev.device)
    if status is not None:
        dev.out["status"][:len(status)] = torch.from_numpy(np.ascontiguousarray(status, np.int32)).to(dev.device)
    dev.keys.fill_(FILL)
    dev.launch_indel_keys()
    res = dev.results()
    return res["indel_keys"], res["hpos"], res["status"], dev


def check(pb, **kw):
    got, hpos, status, _dev = device_keys(pb, **kw)
    want = capi.indel_keys_host(pb, hpos, status, nthreads=4)
    if not np.array_equal(got, want):
        p = int(np.argwhere(got != want)[0][0])
        sl = [s for q, _g, s in cc.pair_hpos_slices(pb) if q == p][0]
        raise AssertionError("pair %d: device %d, host %d, hpos %s" % (p, got[p], want[p], list(hpos[sl])))
    return got, hpos, status


@pytest.mark.parametrize("cfg", [dict(n=6, H=4, R=40, L=36, hap_len=120, max_indel=3), dict(n=5, H=5, R=60, L=100, hap_len=130, vary_read_len=True, mixed_quals=True, max_indel=5),
                                 dict(n=3, H=3, R=24, L=300, hap_len=260, vary_read_len=True, max_indel=5)])
def test_hpos_of_the_faster_kernel(cfg):
    """(a) behind dd_launch_device_faster on seeded batches whose reads carry insertions and deletions against their haplotypes; reads of
    36..300 bp (one and more 64-base chunks, ragged tails)."""
    cfg = dict(cfg)
    pb = synth.generate(cfg.pop("n"), seed=4321 + cfg["L"], **cfg)
    got, hpos, status = check(pb)
    assert (status == 0).all() and (got >= 1).sum() > pb.n_pairs // 20 and (got >= 0).all()
    assert np.array_equal(got, ik.expected(pb, hpos))                       # ... and the Python restatement, while the arrays are at hand


def test_hpos_of_a_ragged_batch():
    pb = synth.generate_ragged(14, seed=99, max_reads=120)
    got, _hpos, _status = check(pb)
    assert (got >= 1).any()


def test_adversarial_alignments():
    """(b) alignments written straight into the device buffer: reads of 1, 2, 63, 64, 65, 128, 129 and 130 bases; deletions and insertion
    runs on and across the chunk ends; runs at the read's ends; bare runs whose lhp comes from an earlier chunk or is the initial 1; the
    same key from several events; non-monotone positions; other negative codes; int16 extremes; exactly 64 and 65 distinct keys."""
    pb, hpos = ik.adversarial_batch()
    got, _hpos, _status = check(pb, hpos=hpos, launch=None)
    want = ik.expected(pb, hpos)
    assert np.array_equal(got, want)
    assert {0, 1, 2, 63, 64, ik.OVERFLOW} <= set(int(v) for v in np.unique(got)) and (got == ik.OVERFLOW).sum() >= 10


def test_pairs_without_likelihood_are_marked_and_their_hpos_is_not_read():
    """(c) a non-zero dd_result.status: DD_INDEL_KEYS_NOT_COMPUTED whatever hpos holds."""
    pb, hpos = ik.adversarial_batch()
    rng = np.random.default_rng(2)
    status = rng.choice([0, 0, 0, capi.DD_PAIR_HAPSIZE, capi.DD_PAIR_NAN, capi.DD_PAIR_LLPOS, capi.DD_PAIR_UNSUPPORTED], pb.n_pairs).astype(np.int32)
    hpos = hpos.copy()
    for p, _g, sl in cc.pair_hpos_slices(pb):
        if status[p]:
            hpos[sl] = rng.integers(-32768, 32768, sl.stop - sl.start)
    got, _hpos, _status = check(pb, hpos=hpos, status=status, launch=None)
    assert (got[status != 0] == ik.NOT_COMPUTED).all() and (got[status == 0] != ik.NOT_COMPUTED).all()
    assert np.array_equal(got, ik.expected(pb, hpos, status))


def _long_window(rng, hap_len, L, R=4):
    hap = "".join(rng.choice(list("ACGT"), hap_len))
    hap2 = hap[:hap_len // 2] + "GT" + hap[hap_len // 2:]
    reads = []
    for _ in range(R):
        off = int(rng.integers(-L // 3, max(1, hap_len - L // 2)))
        src = hap2 if rng.random() < 0.5 else hap
        seq = "".join(src[i] if 0 <= i < len(src) else "A" for i in range(off, off + L))
        reads.append(ReadRec(seq, [0.999] * L, 0.9999, 1000 + off))
    return Window(1000, [hap, hap2], reads)


def long_batch():
    rng = np.random.default_rng(31)
    return pack([_long_window(rng, 900, 150), _long_window(rng, 300, 1100, R=1), _long_window(rng, 200, 100)])


def test_behind_the_faster_long_launch():
    """(d) one 1,100-base read (18 chunks) and a 900-bp haplotype, computed by dd_launch_device_faster_long; without the option their pairs
    are not computed and are marked."""
    pb = long_batch()
    got, _hpos, status = check(pb, long_windows_faster=True)
    assert (status == 0).all() and (got >= 0).all()
    got, _hpos, status = check(pb)
    assert (got == ik.NOT_COMPUTED).sum() == 2 * 4 + 2 * 1 and ((got == ik.NOT_COMPUTED) == (status != 0)).all()


def test_more_pairs_than_the_grid_has_wavefronts():
    """(e) the grid is persistent (2,048 workgroups x 4 wavefronts): 3 rounds and a partial one."""
    rng = np.random.default_rng(6)
    pb = cc.csr_batch([([200, 200, 200], [int(rng.integers(1, 90)) for _ in range(230)]) for _ in range(40)])
    assert pb.n_pairs > 3 * 2048 * 4
    reads = ik.adversarial_reads(n_random=100)
    hpos = np.zeros(pb.hpos_len, np.int16)
    for _p, _g, sl in cc.pair_hpos_slices(pb):
        L = sl.stop - sl.start
        src = reads[int(rng.integers(0, len(reads)))]
        hpos[sl] = np.resize(np.asarray(src, np.int16), L)
    got, _hpos, _status = check(pb, hpos=hpos, launch=None)
    assert (got == ik.OVERFLOW).any() and (got > 0).sum() > pb.n_pairs // 2


def test_on_a_stream_of_its_own_and_launched_again_into_the_same_tensors():
    """(f) a non-default stream; a second launch over other alignments overwrites every pair of the first."""
    pb, hpos = ik.adversarial_batch()
    dev = DeviceBatch(pb, capi.params_cli_defaults(), "cuda:0", indel_keys=True)
    s = torch.cuda.Stream(device=dev.device)
    other = hpos[::-1].copy()
    with torch.cuda.stream(s):
        dev.out["hpos"][:len(hpos)] = torch.from_numpy(hpos).to(dev.device)
        dev.keys.fill_(FILL)
        dev.launch_indel_keys(stream=s)
        first = dev.keys.clone()
        dev.out["hpos"][:len(hpos)] = torch.from_numpy(other).to(dev.device)
        dev.launch_indel_keys(stream=s)
    s.synchronize()
    assert np.array_equal(first[:pb.n_pairs].cpu().numpy(), capi.indel_keys_host(pb, hpos))
    assert np.array_equal(dev.results()["indel_keys"], capi.indel_keys_host(pb, other))


def host_entry(lib, pb, options=0, with_hpos=False):
    p = capi.params_cli_defaults()
    arrs, res = alloc_result(pb)
    if not with_hpos:
        res.hpos = None
        arrs["hpos"][:] = -12345
    out = np.full(pb.n_pairs, FILL, np.int16)
    b = pb.ctypes_batch()
    rc = lib.dd_compute_likelihoods_faster_keys(C.byref(p), C.byref(b), C.byref(res), out.ctypes.data_as(capi.c_i16p), 0, options)
    assert rc == 0, capi.last_error()
    return out, arrs


def plain_faster(lib, pb, options=0):
    p = capi.params_cli_defaults()
    arrs, res = alloc_result(pb)
    b = pb.ctypes_batch()
    assert lib.dd_compute_likelihoods_faster_ex(C.byref(p), C.byref(b), C.byref(res), 0, options) == 0, capi.last_error()
    return arrs


def test_host_entry_keeps_the_alignments_on_the_device(lib):
    """(g) dd_compute_likelihoods_faster_keys with r->hpos == NULL: the counts of the alignments a plain call brings back, the other outputs
    of dd_compute_likelihoods_faster, and no alignment copied back; asking for the alignments as well changes nothing else; the same
    with DD_OPT_LONG_WINDOWS_FASTER."""
    pb = synth.generate(5, H=5, R=60, L=100, hap_len=130, seed=1334, vary_read_len=True, mixed_quals=True, max_indel=5)
    plain = plain_faster(lib, pb)
    want = capi.indel_keys_host(pb, plain["hpos"], plain["status"])
    assert (want >= 1).any()
    got, arrs = host_entry(lib, pb)
    assert np.array_equal(got, want) and (arrs["hpos"] == -12345).all()
    for k in plain:
        if k != "hpos":
            assert np.array_equal(plain[k], arrs[k]), k
    got2, arrs2 = host_entry(lib, pb, with_hpos=True)
    assert np.array_equal(got2, want) and np.array_equal(arrs2["hpos"], plain["hpos"])
    pbl = long_batch()
    plainl = plain_faster(lib, pbl, capi.DD_OPT_LONG_WINDOWS_FASTER)
    assert (plainl["status"] == 0).all()
    gotl, arrsl = host_entry(lib, pbl, options=capi.DD_OPT_LONG_WINDOWS_FASTER)
    assert np.array_equal(gotl, capi.indel_keys_host(pbl, plainl["hpos"], plainl["status"])) and np.array_equal(arrsl["ll"], plainl["ll"])
    gots, _ = host_entry(lib, pbl)                                           # without the option the long windows' pairs are marked
    assert (gots == ik.NOT_COMPUTED).sum() == 2 * 4 + 2 * 1


def test_host_entry_in_window_blocks(lib):
    """A batch of more than a million pairs runs as window blocks on two streams: every block's counts arrive, equal to the
    device-pointer path's."""
    small = synth.generate(8, H=8, R=200, L=60, hap_len=100, seed=5, max_indel=3)
    pb = synth.tile(small, 90)
    assert pb.n_pairs > 1100000
    ref, _hpos, _status, _dev = device_keys(pb)
    assert (ref >= 1).any() and (ref >= 0).all()
    got, _ = host_entry(lib, pb)
    assert np.array_equal(got, ref)
    n0 = int(small.win_pair_off[1])                                          # the first window against the CPU evaluation
    assert np.array_equal(got[:n0], capi.indel_keys_host(small.slice_windows(0, 1), _hpos[:int(small.win_hpos_off[1])]))
