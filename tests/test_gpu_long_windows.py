"""GPU: the long-window path (DD_OPT_LONG_WINDOWS) against the CPU oracle, every dd_result field bit-equal.

Windows the main kernels do not cover — haplotypes of 767..4,094 bp, reads of 1,025..4,096 bp, haplotypes of 575..766 bp at
maxLengthDel 12..31 — go to the long kernel (one workgroup per pair, K = 1, 2, 4, 8, 16 states per thread: numS <= 256 K) when the
option is set; without it they stay DD_PAIR_UNSUPPORTED.
"""
import ctypes as C

import numpy as np
import pytest

from dindel_tgi_amd import capi, synth
from dindel_tgi_amd.batch import ReadRec, Window, alloc_result, pack
from tests import _oracle
from tests.test_gpu_parity import INT_KEYS, F64_KEYS, assert_same, run_host_api

pytestmark = pytest.mark.gpu
RNG = np.random.default_rng(20261016)


def rnd(n, alphabet="ACGT"):
    return "".join(RNG.choice(list(alphabet), n))


def mutate(s, rate=0.005):
    out = list(s)
    for i in range(len(out)):
        if RNG.random() < rate:
            out[i] = RNG.choice(list("ACGT"))
    return "".join(out)


def reads_from(hap, n, L, start0=1000, q=0.999, mq=0.9999, junk=0.0, rate=0.005):
    reads = []
    for _ in range(n):
        off = int(RNG.integers(-L // 2, max(1, len(hap) - L // 2)))
        seq = "".join(hap[i] if 0 <= i < len(hap) else RNG.choice(list("ACGT")) for i in range(off, off + L))
        if RNG.random() < junk:
            seq = rnd(L)
        reads.append(ReadRec(mutate(seq, rate), [q] * L, mq, start0 + off))
    return reads


def run_ex(lib, params, pb, options=capi.DD_OPT_LONG_WINDOWS):
    arrs, res = alloc_result(pb, fill=None)
    b = pb.ctypes_batch()
    rc = lib.dd_compute_likelihoods_ex(C.byref(params), C.byref(b), C.byref(res), 0, options)
    assert rc == 0, capi.last_error()
    return arrs


def params(mld=5, **kw):
    p = capi.params_cli_defaults()
    p.maxLengthDel = mld
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def check(lib, p, pb, nthreads=16):
    cls, _mx, _n = capi.screen_windows_ex(p, pb)
    got = run_ex(lib, p, pb)
    assert_same(got, _oracle.batch(p, pb, nthreads=nthreads), pb)
    return got, cls


# (hap_len, read_len, maxLengthDel, haplotypes, reads per window): 767 bp; the K steps 4 -> 8 -> 16 (numS = 256 K and 256 K + 1; 1 -> 2 and
# 2 -> 4 in test_k_boundaries); 4,094 bp;
# reads from 36 bp (against long haplotypes) up to 4,096 bp (against short ones); 575..766 bp at maxLengthDel 12..31
SHAPES = [(767, 150, 5, 3, 6), (1022, 120, 0, 2, 4), (1023, 120, 11, 2, 4), (2046, 36, 12, 2, 5), (2047, 150, 20, 2, 3),
          (3000, 250, 31, 2, 2), (4094, 300, 5, 2, 2), (120, 1025, 5, 3, 3), (254, 1500, 11, 2, 2), (255, 2000, 20, 1, 2),
          (60, 4096, 5, 1, 2), (575, 100, 12, 3, 5), (700, 130, 20, 3, 4), (766, 150, 31, 3, 4), (574, 1100, 31, 2, 2)]


@pytest.mark.parametrize("shape", SHAPES, ids=["h%d_r%d_d%d" % s[:3] for s in SHAPES])
def test_long_shapes_match_oracle(lib, shape):
    hs, L, mld, H, R = shape
    pb = synth.generate(2, H=H, R=R, L=L, hap_len=hs, seed=hs * 7 + L, max_indel=max(1, mld), sub_rate=0.004, vary_read_len=L <= 1024,
                        mixed_quals=True)
    _got, cls = check(lib, params(mld), pb)
    assert (cls == capi.DD_WIN_LONG).all(), cls
    log = capi.long_launch_log()
    assert len(log) == 1 and log[0]["pairs"] == pb.n_pairs
    numS = max(pb.max_hap_len, 1) + 2
    assert 256 * log[0]["K"] >= numS and (log[0]["K"] == 1 or 128 * log[0]["K"] < numS)


@pytest.mark.parametrize("hs,K", [(254, 1), (255, 2), (510, 2), (511, 4)])
def test_k_boundaries(lib, hs, K):
    """numS = 256 K is the last shape of a K, 256 K + 1 the first of the next: haplotypes of exactly 254 / 255 / 510 / 511 bp (the longest
    of the window) with reads over 1,024 bp, so that the window goes to the long path."""
    hap = rnd(hs)
    m = hs // 2
    ws = [Window(1000, [hap, hap[:m] + hap[m + 5:], hap[:m] + "TG" + hap[m + 2:]], reads_from(hap, 3, 1100) + reads_from(hap, 3, 120))]
    assert max(len(h) for h in ws[0].haps) == hs
    pb = pack(ws)
    check(lib, params(11), pb)
    log = capi.long_launch_log()
    assert len(log) == 1 and log[0]["K"] == K


def test_maximum_shape(lib):
    """4,094-bp haplotype x 4,096-bp read (the 16 MiB back-pointer tile), and the 4,094 x 4,096 window next to it at maxLengthDel 31."""
    hap = rnd(4094)
    hap2 = hap[:2000] + hap[2031:]
    ws = [Window(1000, [hap, hap2], reads_from(hap, 1, 4096) + reads_from(hap2, 1, 3000))]
    pb = pack(ws)
    check(lib, params(31), pb, nthreads=2)


def test_junk_and_repeat_reads(lib):
    """Junk reads (RO / LO win the join), tandem repeats (near-ties: the serial replay of the scan) and reads that slide off both ends."""
    unit = "ACGTTGCA"
    rep = (unit * 200)[:1500]
    hap = rnd(300) + rep + rnd(300)
    ws = [Window(5000, [hap, hap[:900] + hap[912:]], reads_from(hap, 4, 200, start0=5000, junk=0.5) +
                 reads_from(hap, 3, 1100, start0=5000, junk=0.3)),
          Window(5000, [(unit * 120)[:900]], reads_from((unit * 120)[:900], 4, 160, start0=5000))]
    pb = pack(ws)
    check(lib, params(5), pb)
    check(lib, params(20), pb)


def test_hapsize_error_in_long_window(lib):
    """A long read against a haplotype shorter than maxLengthDel: "hapSize error." for that haplotype's pairs, the others computed."""
    long_hap = rnd(900)
    ws = [Window(1000, [rnd(10), long_hap], reads_from(long_hap, 3, 1100) + reads_from(long_hap, 2, 80))]
    pb = pack(ws)
    got, _ = check(lib, params(20), pb)
    st = got["status"][:pb.n_pairs]
    assert (st[:5] == capi.DD_PAIR_HAPSIZE).all() and (st[5:] == 0).all()


@pytest.mark.parametrize("bmid", [-1, 0, 5000])
def test_unmapped_reads_and_bmid_corners(lib, bmid):
    hap = rnd(1200)
    reads = reads_from(hap, 4, 150)
    reads[0].unmapped = True
    reads[1].start = 10 ** 6                            # far right of the haplotype: bMid = L / 2
    reads[2].start = 0xFFFFFF00                         # uint32 arithmetic of Init (readEnd wraps)
    reads += reads_from(hap, 2, 1300)
    pb = pack([Window(1000, [hap, hap[:600] + hap[607:]], reads)])
    check(lib, params(11, bMid=bmid), pb)


def test_map_unmapped_reads_with_mates(lib):
    """mapUnmappedReads: the library insert-size prior at the join (mate position / length, both orientations, several libraries)."""
    hap = rnd(1500)
    reads = reads_from(hap, 6, 140) + reads_from(hap, 2, 1100)
    for i, r in enumerate(reads):
        r.paired = True
        r.mate_same_tid = i % 4 != 3
        r.mate_reverse = i % 2 == 0
        r.mate_unmapped = i == 5
        r.mate_pos = 1000 + 300 * i
        r.mate_len = 100 if i != 4 else -1
        r.lib = i % 2
    libs = [(np.full(400, 1.0 / 400), 1.0 / 400), (np.linspace(1, 2, 900) / np.linspace(1, 2, 900).sum(), 0.5 / 900)]
    pb = pack([Window(1000, [hap, hap[:700] + "GATTACA" + hap[700:]], reads)], libraries=libs)
    check(lib, params(5, mapUnmappedReads=1), pb)


def test_coverage_flags_and_odd_bytes(lib):
    """hap_var + hap_var_flank coverage flags, IUPAC and soft-masked bytes on both sides ('N' a wildcard on the haplotype only)."""
    ref = rnd(1000)
    hap_del = ref[:500] + ref[530:]
    hap_ins = ref[:500] + "TTTT" + ref[500:]
    odd = ref[:100] + "NRYk" + ref[104:300].lower() + ref[300:]
    reads = reads_from(ref, 6, 150) + reads_from(hap_del, 5, 150) + reads_from(hap_ins, 4, 150)
    reads[0] = ReadRec("NNRY" + reads[0].seq[4:].lower(), reads[0].qual, reads[0].mapQual, reads[0].start)
    w = Window(1000, [ref, hap_del, hap_ins, odd], reads,
               hap_vars=[[], [(499, 500)], [(500, 503)], [(100, 103)]],
               hap_var_flanks=[[], [(499, 500, 1)], [(499, 504, 2)], [(100, 103, 0)]])
    pb = pack([w])
    check(lib, params(31), pb)
    check(lib, params(5, padCover=0, maxMismatch=0), pb)


def test_mixed_batch_main_long_and_unsupported(lib):
    """Normal, long and still-unsupported windows in one batch: long = oracle, normal byte-identical to the plain call, unsupported as today."""
    p = params(5)

    def normal(hs, R):
        h = rnd(hs)
        m = hs // 2
        return Window(1000, [h, h[:m] + h[m + 3:], h[:m] + "AC" + h[m:]], reads_from(h, R, 100),
                      hap_vars=[[], [(m - 1, m)], [(m, m + 1)]], hap_var_flanks=[[], [(m - 1, m, 1)], [(m - 1, m + 2, 2)]])
    hap = rnd(1400)
    ws = [normal(150, 30), normal(200, 25), normal(120, 20),
          Window(1000, [hap, hap[:700] + hap[703:]], reads_from(hap, 5, 150)),
          Window(1000, [rnd(4095)], reads_from(rnd(200), 2, 100)), Window(1000, [rnd(300)], reads_from(rnd(300), 2, 4097)),
          Window(1000, [rnd(1000)], [ReadRec("", [], 0.9999, 1000)] + reads_from(rnd(300), 1, 90)),
          normal(140, 20), normal(700, 10)]
    pb = pack(ws)
    cls, _mx, n_bad = capi.screen_windows_ex(p, pb)
    assert list(cls) == [0, 0, 0, 2, 1, 1, 1, 0, 0] and n_bad == 3
    got = run_ex(lib, p, pb)
    plain = run_host_api(lib, p, pb)
    want = _oracle.batch(p, pb, nthreads=16, first_window=3, n_win=1)
    po, ho, ro, vo = pb.win_pair_off, pb.win_hpos_off, pb.a["win_read_off"], pb.win_varcov_off
    assert pb.var_cov_len > 0
    for w in range(pb.n_windows):
        ps, hs_, rs, vs = slice(po[w], po[w + 1]), slice(ho[w], ho[w + 1]), slice(ro[w], ro[w + 1]), slice(vo[w], vo[w + 1])
        if cls[w] == 0:
            for k in INT_KEYS + F64_KEYS:
                sl = hs_ if k == "hpos" else (rs if k == "onHap" else (vs if k in ("var_covered", "var_fcov") else ps))
                assert got[k][sl].tobytes() == plain[k][sl].tobytes(), (w, k)
        elif cls[w] == 2:
            for k in ("ll", "llOn", "llOff", "mLogBQ", "status", "offHap", "offHapHMQ", "numIndels", "numMismatch", "nBQT", "nmmBQT",
                      "nMMLeft", "nMMRight", "firstBase", "lastBase"):
                assert got[k][ps].tobytes() == want[k][ps].tobytes(), (w, k)
            assert np.array_equal(got["hpos"][hs_], want["hpos"][hs_])
            assert np.array_equal(got["onHap"][rs], want["onHap"][rs])
            assert (plain["status"][ps] == capi.DD_PAIR_UNSUPPORTED).all()
        else:
            assert (got["status"][ps] == capi.DD_PAIR_UNSUPPORTED).all() and (got["ll"][ps] == 0).all()
            assert (got["offHap"][ps] == 1).all() and (got["onHap"][rs] == 0).all()


def test_575_to_766_at_large_maxlengthdel_no_longer_fails_the_batch(lib):
    """maxLengthDel 12..31 with a 575..766-bp haplotype: the plain call fails the whole batch, the option computes it."""
    p = params(20)
    pb = synth.concat([synth.generate(2, H=3, R=10, L=100, hap_len=200, seed=9), synth.generate(1, H=2, R=6, L=120, hap_len=650, seed=10)])
    arrs, res = alloc_result(pb, fill=None)
    b = pb.ctypes_batch()
    rc = lib.dd_compute_likelihoods(C.byref(p), C.byref(b), C.byref(res), 0)
    assert rc != 0
    assert lib.dd_compute_likelihoods_ex(C.byref(p), C.byref(b), C.byref(res), 0, 0) == rc
    check(lib, p, pb)


def test_device_pointer_path_equals_host_path(lib):
    from dindel_tgi_amd.device import DeviceBatch
    p = params(12)
    hap, h6 = rnd(2100), rnd(600)
    pb = pack([Window(1000, [h, h[:70] + h[72:], h[:70] + "T" + h[70:]], reads_from(h, 20, 100)) for h in (rnd(150), rnd(160))] +
              [Window(1000, [hap, hap[:1000] + hap[1010:]], reads_from(hap, 6, 150) + reads_from(hap, 2, 1200)),
               Window(1000, [h6, h6[:300] + h6[313:]], reads_from(h6, 8, 100))])
    host = run_ex(lib, p, pb)
    dev = DeviceBatch(pb, p, "cuda:0", long_windows=True)
    assert dev.n_long == 2
    dev.launch()
    got = dev.results()
    for k, _ in capi.RESULT_FIELDS:
        n = len(got[k])
        assert got[k].tobytes() == host[k][:n].tobytes(), k
    log = capi.long_launch_log()
    assert len(log) == 1 and log[0]["pairs"] == 2 * 8 + 2 * 8
    # without the flag the device path marks them, as before
    dev0 = DeviceBatch(pb, p, "cuda:0")
    assert dev0.n_long == 0


def test_more_pairs_than_the_grid_holds(lib):
    """A persistent grid: some workgroup takes two pairs or more (the launch record), every pair still equal to the oracle."""
    p = params(5)
    pb = synth.generate(4, H=4, R=48, L=90, hap_len=1000, seed=31, mixed_quals=True)
    check(lib, p, pb, nthreads=16)
    log = capi.long_launch_log()
    assert len(log) == 1
    assert log[0]["pairs"] == pb.n_pairs and pb.n_pairs > log[0]["grid"]
    assert log[0]["max_pairs_per_wg"] >= 2
    assert log[0]["ws_bytes"] <= capi.DD_LONG_WS_BUDGET
