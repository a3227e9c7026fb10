"""What the side kernels' host entries share (csrc/capi_internal.h: the launch record, the one-shot arena): the three launches behind an
alignment keep their header words apart, a record survives the workspace of a host-pointer entry as cached values and no longer leads
to it, and arrays of 0 bytes have an address in the arena.  The shapes are the smallest that take more than one workgroup."""
import random

import numpy as np
import pytest

from dindel_tgi_amd import capi, hapalign, hapdist, pooled
from tests import _haplotypes_cases as hc
from tests.test_gpu_pooled_em import assert_same_bits, mask

pytestmark = pytest.mark.gpu
HAP_LENS = [5, 70, 12, 33, 64, 48, 7, 25, 59]       # nine pairs: three workgroups of four wavefronts; one haplotype longer than 64 bases
CAP = 4


def nine_pairs():
    rng = random.Random(9)
    refs = [bytes(rng.choice(b"ACGT") for _ in range(n)) for n in (40, 60)]
    pair_ref = [i % 2 for i in range(len(HAP_LENS))]
    haps = []
    for r, n in zip(pair_ref, HAP_LENS):
        s = bytearray((refs[r] * 2)[3:3 + n])           # a piece of the reference (taken round its end where it is longer) with an
        s[n // 2] = b"ACGT"[(b"ACGT".index(s[n // 2]) + 1) % 4]   # exchange, so that events and variants have something to report
        if n > 10:
            del s[3:5]
            s[8:8] = b"GA"
        haps.append(bytes(s))
    assert [len(h) for h in haps] == HAP_LENS
    return refs, haps, pair_ref


@pytest.fixture(scope="module")
def host_results():
    """The three host-pointer entries on the nine pairs."""
    refs, haps, pair_ref = nine_pairs()
    return {"plain": hapalign.align_haplotypes(refs, haps, pair_ref), "events": hapalign.align_events(refs, haps, pair_ref, events_cap=CAP),
            "variants": hapalign.align_variants(refs, haps, pair_ref, cap=CAP)}


def check_record(log, n=9, grid=3, items="pairs"):
    assert log[items] == n and log["grid"] == grid and 1 <= log["max_draws"] <= n and log["guard_trips"] == 0, log


def test_three_launches_behind_each_other_keep_their_words_apart(host_results):
    import torch
    dev = hapalign.DeviceAlign(*nine_pairs(), "cuda:0")
    st = torch.cuda.Stream(device="cuda:0")
    dev.launch(st)
    dev.launch_events(CAP, st)
    dev.launch_variants(CAP, st)
    for read in (hapalign.variants_last_launch, hapalign.events_last_launch, hapalign.last_launch):
        log = read()
        print(read.__name__, log)
        check_record(log)
        assert read() == log                        # a second reading finds the cached words
    got = dev.results()
    for k in ("score", "status", "ref_pos"):
        assert np.array_equal(got[k], host_results["plain"][k]), k
    assert (got["status"] == capi.DD_ALIGN_OK).all()
    ev, va = dev.event_results(), dev.variant_results()
    for k in ("n_events", "events"):
        assert np.array_equal(ev[k], host_results["events"][k]), k
    for k in ("summary", "variants"):
        assert np.array_equal(va[k], host_results["variants"][k]), k
    # the pairs do hold something: the events tests/_candidates_oracle.py counts in the rows of tests/_hapalign_oracle.py, and variants
    assert ev["n_events"].tolist() == [0, 2, 2, 2, 0, 2, 0, 2, 2] and va["summary"][:, 0].max() >= 1


@pytest.mark.parametrize("entry", ["plain", "events", "variants"])
def test_a_host_pointer_entry_leaves_cached_records_and_no_workspace(entry):
    refs, haps, pair_ref = nine_pairs()
    dev = hapalign.DeviceAlign(refs, haps, pair_ref, "cuda:0")      # valid device arrays for the two entries that must refuse
    if entry == "plain":
        hapalign.align_haplotypes(refs, haps, pair_ref)
        readers = [hapalign.last_launch]
    elif entry == "events":
        hapalign.align_events(refs, haps, pair_ref, events_cap=CAP)
        readers = [hapalign.last_launch, hapalign.events_last_launch]
    else:
        hapalign.align_variants(refs, haps, pair_ref, cap=CAP)
        readers = [hapalign.last_launch, hapalign.variants_last_launch]
    for read in readers:                                # the workspace went with the call: these are the values it cached
        log = read()
        print(entry, read.__name__, log)
        assert log["pairs"] == 9 and log["max_draws"] >= 1, log
        check_record(log)
        assert read() == log
    with pytest.raises(RuntimeError, match="dd_align_events_device: .*no alignment launch"):
        dev.launch_events(CAP)
    with pytest.raises(RuntimeError, match="dd_hap_variants_device: .*no alignment launch"):
        dev.launch_variants(CAP)


def nine_windows():
    windows, reads = [], []
    for i in range(9):
        rs = 1000 + 40 * i
        windows.append((rs, hc.G[rs:rs + 20]))
        texts = [(rs, "20M"), (rs + 2, "6M2I8M"), (rs + 4, "5M3D8M")]
        reads.append([(pos, 0, hc.cigar(t), hc.read_from(hc.G, pos, hc.cigar(t), random.Random(pos), 0.1)) for pos, t in texts])
    return windows, reads


def test_block_table_record_after_the_host_entry_and_on_a_stream():
    import torch
    windows, reads = nine_windows()
    a, want = hapdist.block_table(windows, reads)
    log = hapdist.last_launch()
    print("block_table", log)
    check_record(log, items="windows")
    assert hapdist.last_launch() == log
    assert (want["status"] == capi.DD_HAPDIST_OK).all() and (want["n_blocks"] == 8).all() and (want["n_ins_ops"] == 1).all()   # as blockTableHost has them
    dev = hapdist.DeviceBlocks(windows, reads, "cuda:0")
    st = torch.cuda.Stream(device="cuda:0")
    dev.launch(st)
    log = hapdist.last_launch()
    print("DeviceBlocks", log)
    check_record(log, items="windows")
    _, got = dev.results()
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def test_pooled_em_with_arrays_of_no_bytes(lib):
    """a window without reads among others; and a slot table whose windows have no haplotypes (F = 0: compat and freqs are empty)"""
    shapes = [(2, 10), (3, 0), (0, 5), (0, 0), (5, 67)]
    rng = np.random.default_rng(5)
    who = np.concatenate([[0], np.cumsum([s[0] for s in shapes])]).astype(np.int32)
    wro = np.concatenate([[0], np.cumsum([s[1] for s in shapes])]).astype(np.int32)
    ll = np.concatenate([rng.uniform(-150.0, -5.0, size=nh * nr) for nh, nr in shapes])
    for sw in ([0, 1, 4, 1, 2], [2, 3, 3]):
        slots = pooled.pack_slots(who, sw, [mask("alternating" if k % 2 else "all", shapes[w][0]) for k, w in enumerate(sw)])
        assert (int(slots["slot_off"][-1]) == 0) == (sw[0] == 2)
        assert_same_bits(pooled.em(who, wro, ll, slots, a0=0.5), pooled.em_host(who, wro, ll, slots, a0=0.5))
    # and no pair at all: ll is empty as well
    who0, wro0 = np.array([0, 2, 2], np.int32), np.array([0, 0, 0], np.int32)
    slots = pooled.pack_slots(who0, [1, 0], [[], [1, 1]])
    assert_same_bits(pooled.em(who0, wro0, np.zeros(0), slots), pooled.em_host(who0, wro0, np.zeros(0), slots))
