"""GPU: the --faster model's long-window path (DD_OPT_LONG_WINDOWS_FASTER) against the CPU oracle (ddo_batch_fast), every dd_result
field bit-equal — the bar dd_faster_kernel is held to in test_gpu_faster.py.

Windows dd_faster_kernel does not cover — haplotypes of 767..4,094 bp, reads of 1,025..4,096 bp — go to faster_long_kernel.hip when the
option is set; without it, and with the main model's DD_OPT_LONG_WINDOWS, they stay DD_PAIR_UNSUPPORTED.
"""
import ctypes as C

import numpy as np
import pytest

from dindel_tgi_amd import capi, synth
from dindel_tgi_amd.batch import ReadRec, Window, alloc_result, pack
from tests import _oracle
from tests.test_gpu_faster import assert_same_faster, run_faster
from tests.test_gpu_long_windows import mutate, params, reads_from, rnd
from tests.test_gpu_parity import F64_KEYS, INT_KEYS, assert_same

pytestmark = pytest.mark.gpu
FL = capi.DD_OPT_LONG_WINDOWS_FASTER


def run_ex(lib, p, pb, options=FL):
    arrs, res = alloc_result(pb, fill=None)
    b = pb.ctypes_batch()
    rc = lib.dd_compute_likelihoods_faster_ex(C.byref(p), C.byref(b), C.byref(res), 0, options)
    assert rc == 0, capi.last_error()
    return arrs


def check(lib, p, pb, nthreads=16):
    """Every field against the oracle: assert_same (test_gpu_parity: all INT_KEYS / F64_KEYS where both sides write them) and the
    --faster comparison of test_gpu_faster (hpos of failed pairs excluded pair by pair)."""
    cls, _mx, _n = capi.screen_windows_ex(p, pb, FL)
    got = run_ex(lib, p, pb)
    want = _oracle.batch(p, pb, faster=True, nthreads=nthreads)
    assert_same_faster(got, want, pb)
    if (want["status"][:pb.n_pairs] == 0).all():
        assert_same(got, want, pb)
    return got, cls


# (hap_len, read_len, maxLengthDel, haplotypes, reads per window)
SHAPES = [(767, 150, 5, 3, 6), (1000, 36, 0, 2, 20), (2000, 100, 5, 2, 40), (3000, 250, 20, 2, 5), (4094, 300, 31, 2, 4),
          (60, 1025, 5, 3, 3), (254, 1500, 0, 2, 5), (1000, 1500, 20, 2, 3), (4094, 1025, 5, 1, 2), (60, 4096, 31, 1, 2)]


@pytest.mark.parametrize("shape", SHAPES, ids=["h%d_r%d_d%d" % s[:3] for s in SHAPES])
def test_long_shapes_match_oracle(lib, shape):
    hs, L, mld, H, R = shape
    mi = max(1, min(mld, 12))                     # an inserted haplotype is up to mi bases longer: stay within 4,094 (exactly 4,094: test_maximum_shape)
    pb = synth.generate(2, H=H, R=R, L=L, hap_len=min(hs, 4094 - mi), seed=hs * 7 + L, max_indel=mi, sub_rate=0.004,
                        vary_read_len=L <= 1024, mixed_quals=True)
    _got, cls = check(lib, params(mld), pb)
    assert (cls == capi.DD_WIN_LONG).all(), cls
    log = capi.faster_long_launch_log()
    assert len(log) == 1 and log[0]["pairs"] == pb.n_pairs and log[0]["grid"] >= 1


def test_maximum_shape(lib):
    hap = rnd(4094)
    hap2 = hap[:2000] + hap[2031:]
    pb = pack([Window(1000, [hap, hap2], reads_from(hap, 2, 4096) + reads_from(hap2, 1, 3000) + reads_from(hap, 2, 150))])
    check(lib, params(5), pb, nthreads=4)


def test_junk_and_tandem_repeats(lib):
    """Junk reads; tandem repeats: ties between diagonals, far more than 15 candidate diagonals, large vote counts."""
    unit = "ACGTTGCA"
    rep = (unit * 200)[:1500]
    hap = rnd(300) + rep + rnd(300)
    mono = "A" * 1200
    ws = [Window(5000, [hap, hap[:900] + hap[912:]], reads_from(hap, 6, 200, start0=5000, junk=0.5) +
                 reads_from(hap, 3, 1100, start0=5000, junk=0.3)),
          Window(5000, [(unit * 120)[:900]], reads_from((unit * 120)[:900], 5, 160, start0=5000)),
          Window(5000, [mono, mono[:-7]], reads_from(mono, 3, 120, start0=5000) + [ReadRec("A" * 1100, [0.99] * 1100, 0.999, 5010)])]
    pb = pack(ws)
    check(lib, params(5), pb)
    check(lib, params(31), pb)


def test_hapsize_error_and_short_read_in_long_window(lib):
    """A haplotype shorter than maxLengthDel next to a long one: "hapSize error." for its pairs only; a 3-bp read: "HapHash string too
    short" for that read's pairs only."""
    long_hap = rnd(900)
    reads = reads_from(long_hap, 3, 1100) + reads_from(long_hap, 2, 80) + [ReadRec("ACG", [0.99] * 3, 0.999, 1100)]
    pb = pack([Window(1000, [rnd(10), long_hap], reads)])
    got, _ = check(lib, params(20), pb)
    st = got["status"][:pb.n_pairs]
    assert (st[:6] == capi.DD_PAIR_HAPSIZE).all() and (st[6:11] == 0).all() and st[11] == capi.DD_PAIR_NAN
    got, _ = check(lib, params(5), pb)
    st = got["status"][:pb.n_pairs]
    assert (st[[5, 11]] == capi.DD_PAIR_NAN).all() and (np.delete(st, [5, 11]) == 0).all()


def test_unmapped_reads_and_bmid_corners(lib):
    hap = rnd(1200)
    reads = reads_from(hap, 6, 150)
    reads[0].unmapped = True
    reads[1].start = 10 ** 6                            # entirely right of the haplotype: bMid = 0
    reads[2].start = 0                                  # entirely left: bMid = L - 1
    reads[3].start = 0xFFFFFF00                         # uint32 arithmetic (readEnd wraps)
    reads += reads_from(hap, 2, 1300)
    reads[-1].start = 10 ** 6
    pb = pack([Window(1000, [hap, hap[:600] + hap[607:]], reads)])
    check(lib, params(11), pb)


def test_coverage_flags_and_odd_bytes(lib):
    """hap_var + hap_var_flank coverage flags, IUPAC and lower-case bytes on both sides (non-ACGT hashes as 'A', bytes are compared)."""
    ref = rnd(1000)
    hap_del = ref[:500] + ref[530:]
    hap_ins = ref[:500] + "TTTT" + ref[500:]
    odd = ref[:100] + "NRYk" + ref[104:300].lower() + ref[300:]
    reads = reads_from(ref, 6, 150) + reads_from(hap_del, 5, 150) + reads_from(hap_ins, 4, 150) + reads_from(odd, 3, 1030)
    reads[0] = ReadRec("NNRY" + reads[0].seq[4:].lower(), reads[0].qual, reads[0].mapQual, reads[0].start)
    w = Window(1000, [ref, hap_del, hap_ins, odd], reads,
               hap_vars=[[], [(499, 500)], [(500, 503)], [(100, 103)]],
               hap_var_flanks=[[], [(499, 500, 1)], [(499, 504, 2)], [(100, 103, 0)]])
    pb = pack([w])
    assert pb.var_cov_len > 0
    check(lib, params(31), pb)
    check(lib, params(5, padCover=0, maxMismatch=0), pb)


def mixed_batch():
    def normal(hs, R):
        h = rnd(hs)
        m = hs // 2
        return Window(1000, [h, h[:m] + h[m + 3:], h[:m] + "AC" + h[m:]], reads_from(h, R, 100),
                      hap_vars=[[], [(m - 1, m)], [(m, m + 1)]], hap_var_flanks=[[], [(m - 1, m, 1)], [(m - 1, m + 2, 2)]])
    hap = rnd(1400)
    m = 700
    ws = [normal(150, 30), normal(200, 25), normal(600, 20),
          Window(1000, [hap, hap[:m] + hap[m + 3:]], reads_from(hap, 37, 150), hap_vars=[[], [(m - 1, m)]], hap_var_flanks=[[], [(m - 1, m, 1)]]),
          Window(1000, [rnd(4095)], reads_from(rnd(200), 2, 100)), Window(1000, [rnd(300)], reads_from(rnd(300), 2, 4097)),
          Window(1000, [rnd(1000)], [ReadRec("", [], 0.9999, 1000)] + reads_from(rnd(300), 1, 90)),
          normal(140, 20), Window(1000, [rnd(300)], reads_from(rnd(300), 3, 1100)), normal(700, 10)]
    return pack(ws), [0, 0, 0, 2, 1, 1, 1, 0, 2, 0]


def test_mixed_batch_main_long_and_unsupported(lib):
    """Ordinary, long and beyond-limit windows in one batch: ordinary byte-identical to dd_compute_likelihoods_faster, long = oracle,
    beyond-limit as today; options = 0 byte-identical to the plain call; maxLengthDel 20 (a 600-bp haplotype stays ordinary)."""
    p = params(20)
    pb, want_cls = mixed_batch()
    cls, _mx, n_bad = capi.screen_windows_ex(p, pb, FL)
    assert list(cls) == want_cls and n_bad == 3
    got = run_ex(lib, p, pb)
    plain = run_faster(lib, p, pb)
    zero = run_ex(lib, p, pb, options=0)
    po, ho, ro, vo = pb.win_pair_off, pb.win_hpos_off, pb.a["win_read_off"], pb.win_varcov_off
    MARKED = ["status", "ll", "offHap", "offHapHMQ", "onHap"]      # all a skipped window's pairs get; its other outputs are not written
    for w in range(pb.n_windows):
        ps, hs_, rs, vs = slice(po[w], po[w + 1]), slice(ho[w], ho[w + 1]), slice(ro[w], ro[w + 1]), slice(vo[w], vo[w + 1])
        for k in (INT_KEYS + F64_KEYS) if cls[w] == 0 else MARKED:
            sl = hs_ if k == "hpos" else (rs if k == "onHap" else (vs if k in ("var_covered", "var_fcov") else ps))
            assert zero[k][sl].tobytes() == plain[k][sl].tobytes(), (w, k)
    for w in range(pb.n_windows):
        ps, hs_, rs, vs = slice(po[w], po[w + 1]), slice(ho[w], ho[w + 1]), slice(ro[w], ro[w + 1]), slice(vo[w], vo[w + 1])
        if cls[w] == 0:
            for k in INT_KEYS + F64_KEYS:
                sl = hs_ if k == "hpos" else (rs if k == "onHap" else (vs if k in ("var_covered", "var_fcov") else ps))
                assert got[k][sl].tobytes() == plain[k][sl].tobytes(), (w, k)
        elif cls[w] == 2:
            want = _oracle.batch(p, pb, faster=True, nthreads=16, first_window=w, n_win=1)
            for k in INT_KEYS + F64_KEYS:
                sl = hs_ if k == "hpos" else (rs if k == "onHap" else (vs if k in ("var_covered", "var_fcov") else ps))
                assert got[k][sl].tobytes() == want[k][sl].tobytes(), (w, k)
            assert (want["status"][ps] == 0).all() and (plain["status"][ps] == capi.DD_PAIR_UNSUPPORTED).all()
        else:
            for k in MARKED:
                sl = rs if k == "onHap" else ps
                assert got[k][sl].tobytes() == plain[k][sl].tobytes(), (w, k)
            assert (got["status"][ps] == capi.DD_PAIR_UNSUPPORTED).all() and (got["ll"][ps] == 0).all()


def test_device_pointer_path(lib):
    import torch
    from dindel_tgi_amd.device import DeviceBatch
    p = params(5)
    pb, want_cls = mixed_batch()
    dev = DeviceBatch(pb, p, "cuda:0", long_windows_faster=True)
    assert dev.n_long == want_cls.count(2) and dev.long_ws_bytes > 0
    dev.launch_faster()
    got = dev.results()
    host = run_ex(lib, p, pb)
    po, ho, ro, vo = pb.win_pair_off, pb.win_hpos_off, pb.a["win_read_off"], pb.win_varcov_off
    for w in range(pb.n_windows):        # (an unsupported window's pairs get status, ll, offHap, offHapHMQ and onHap only: the rest is not written)
        ps, hs_, rs, vs = slice(po[w], po[w + 1]), slice(ho[w], ho[w + 1]), slice(ro[w], ro[w + 1]), slice(vo[w], vo[w + 1])
        for k in (INT_KEYS + F64_KEYS) if want_cls[w] != 1 else ["status", "ll", "offHap", "offHapHMQ", "onHap"]:
            sl = hs_ if k == "hpos" else (rs if k == "onHap" else (vs if k in ("var_covered", "var_fcov") else ps))
            assert got[k][sl].tobytes() == host[k][sl].tobytes(), (w, k)
    log = capi.faster_long_launch_log()
    assert len(log) == 1 and log[0]["pairs"] == 2 * 37 + 3
    with pytest.raises(RuntimeError):
        dev.launch()
    with pytest.raises(ValueError):
        DeviceBatch(pb, p, "cuda:0", long_windows=True, long_windows_faster=True)
    # too small a workspace is an error, not a fault
    rc = lib.dd_launch_device_faster_long(C.byref(p), C.byref(dev.db), C.byref(dev.dr), C.c_void_p(dev.long_ws.data_ptr()), dev.long_ws_bytes - 1,
                                          C.c_void_p(torch.cuda.current_stream(dev.device).cuda_stream))
    assert rc == capi.DD_ERR_INVALID
    # the main model's option keeps having no effect on this model: long windows stay DD_PAIR_UNSUPPORTED
    dev1 = DeviceBatch(pb, p, "cuda:0", long_windows=True)
    dev1.launch_faster()
    got1 = dev1.results()
    plain = run_faster(lib, p, pb)
    po = pb.win_pair_off
    for k in ("status", "ll", "offHap", "offHapHMQ", "onHap"):            # what an unsupported window's pairs get; the rest: ordinary windows
        assert got1[k].tobytes() == plain[k][:len(got1[k])].tobytes(), k
    for k in ("firstBase", "lastBase"):
        assert got1[k][:po[3]].tobytes() == plain[k][:po[3]].tobytes(), k
    assert (got1["status"][po[3]:po[4]] == capi.DD_PAIR_UNSUPPORTED).all()


def test_more_pairs_than_the_grid_holds(lib):
    """One 900-bp haplotype pair x 20,000 short reads: 40,000 pairs, more 16-pair items than resident workgroups, so workgroups draw
    several items from the counter."""
    hap = rnd(900)
    reads = reads_from(hap, 20000, 40)
    pb = pack([Window(1000, [hap, hap[:450] + hap[452:]], reads)])
    p = params(5)
    got = run_ex(lib, p, pb)
    log = capi.faster_long_launch_log()
    assert len(log) == 1, log
    rec = log[0]
    assert rec["pairs"] == pb.n_pairs == 40000
    assert 1 <= rec["grid"] <= 512 and rec["grid"] * 16 < rec["pairs"]
    assert rec["max_items_per_wg"] >= 2 and rec["max_pairs_per_wg"] > 16
    want = _oracle.batch(p, pb, faster=True, nthreads=16)
    assert_same_faster(got, want, pb)
    assert_same(got, want, pb)
