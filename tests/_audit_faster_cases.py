"""What the tests of the --faster model's audit share (helper; no tests in here): a restatement of its comparison rule in numpy, written
unlike csrc/faster_shadow.h's au_compared_faster (masks over whole arrays instead of a walk over pairs), scenario batches with one oracle
run each, and the hand-made pairs for the places the model can go wrong.

The rule (include/dindel_hmm.h, "audit of the --faster model"): status first; both DD_PAIR_OK: the 14 per-pair values, the pair's hpos, its
var_covered and, with hap_var_flank, its var_fcov; both DD_PAIR_NAN or both DD_PAIR_HAPSIZE: ll, llOn ... nMMRight and the coverage bytes,
NOT firstBase, lastBase and hpos, which the kernels never write for such a pair; anything else nothing more."""
import ctypes as C
import functools

import numpy as np

from dindel_tgi_amd import capi
from tests import _audit_cases as ac
from tests import _path_scenarios as ps

ONLY_COMPUTED = ("firstBase", "lastBase", "hpos")                 # fields a pair owns only when it was computed
THROWN = (capi.DD_PAIR_NAN, capi.DD_PAIR_HAPSIZE)
SHADOW_POISON = 0x3C


def faster_classes(p, pb, long_windows=False):
    """The classes the --faster launch screens the batch into: dd_screen_windows_ex with DD_OPT_LONG_WINDOWS_FASTER, or dd_screen_windows."""
    if long_windows:
        return capi.screen_windows_ex(p, pb, capi.DD_OPT_LONG_WINDOWS_FASTER)[0][:pb.n_windows]
    return ac.main_classes(capi.load(), p, pb)


def eligible_windows(pb, cls, long_windows=False):
    ok = (cls == capi.DD_WIN_MAIN) | ((cls == capi.DD_WIN_LONG) if long_windows else False)
    return np.nonzero(ok & (np.diff(pb.win_pair_off) > 0))[0]


def expected_compared(pb, status, chosen, has_flank):
    """-> {field: elements an audit of the windows `chosen` compares}, from the pairs' statuses (both sides equal) and the rule."""
    st = np.asarray(status[:pb.n_pairs])
    in_sample = np.isin(ac.window_of_pairs(pb), chosen)
    ok = in_sample & (st == capi.DD_PAIR_OK)
    owned = in_sample & (ok | np.isin(st, THROWN))
    elem = ps.element_pairs(pb)
    out = {k: int((ok if k in ONLY_COMPUTED else owned).sum()) for k in capi.AUDIT_FIELDS[:15]}
    out["status"] = int(in_sample.sum())
    out["hpos"] = int(ok[elem["hpos"][:pb.hpos_len]].sum())
    out["var_covered"] = int(owned[elem["var_covered"][:pb.var_cov_len]].sum())
    out["var_fcov"] = out["var_covered"] if has_flank else 0
    return out


def shadow_lengths(smp):
    n = {k: int(smp.sizes.n_pairs) for k in capi.AUDIT_FIELDS[:15]}
    n.update(hpos=int(smp.sizes.hpos_len), var_covered=int(smp.sizes.var_cov_len), var_fcov=int(smp.sizes.var_cov_len))
    return n


def poisoned_shadow(smp, poison=SHADOW_POISON):
    """Host arrays of exactly the sample's lengths (one element where a length is 0), every byte `poison`."""
    from dindel_tgi_amd.batch import RESULT_DTYPES
    return {k: np.full(max(n, 1) * np.dtype(RESULT_DTYPES[k]).itemsize, poison, np.uint8).view(RESULT_DTYPES[k]) for k, n in shadow_lengths(smp).items()}


def owned_shadow(pb, smp, want):
    """-> ({field: expected shadow}, {field: mask of the shadow's elements the rule names}) from the oracle's arrays of the --faster model
    (which hold, for a pair the reference throws for, what the library defines: ll 0, offHapHMQ 1, coverage bytes 0)."""
    elem = ps.element_pairs(pb)
    sh = ac.shadow_from(pb, smp, want)
    st = sh["status"][:smp.sizes.n_pairs]
    assert np.isin(st, (capi.DD_PAIR_OK,) + THROWN).all()
    ok = st == capi.DD_PAIR_OK
    pair_of = ac.shadow_from(pb, smp, {k: (elem[k] if k in ac.PER_ELEMENT else np.arange(pb.n_pairs)) for k, _t in capi.RESULT_FIELDS if k != "onHap"})
    shift = np.zeros(pb.n_pairs, np.int64)
    for w in smp.chosen:
        shift[int(pb.win_pair_off[w]):int(pb.win_pair_off[w + 1])] = int(smp.pair_off[w]) - int(pb.win_pair_off[w])
    mask = {}
    for k, n in shadow_lengths(smp).items():
        own = pair_of[k][:n] + shift[pair_of[k][:n]]
        mask[k] = ok[own] if k in ONLY_COMPUTED else np.ones(n, bool)
        sh[k] = sh[k][:n]
    return sh, mask


def assert_shadow_is_the_oracles(got, exp, mask, poison=None):
    """Every element the rule names bit-equal to the oracle's; with `poison`, every other element still holds it in every byte."""
    for k, m in mask.items():
        g = got[k][:len(m)]
        raw, want = g.view(np.uint8).reshape(len(g), -1), exp[k].view(np.uint8).reshape(len(g), -1)
        bad = np.nonzero(m & (raw != want).any(axis=1))[0]
        assert bad.size == 0, "shadow %s[%d] is %r, the oracle has %r (%d elements differ)" % (k, int(bad[0]), g[bad[0]], exp[k][bad[0]], bad.size)
        if poison is not None:
            assert (raw[~m] == poison).all(), "shadow %s: an element outside the rule was written" % k


def oracle(p, pb):
    from tests import _oracle
    want = _oracle.batch(p, pb, nthreads=16, faster=True)
    for a in want.values():
        a.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def scenario(hap_len=126, read_len=36, mld=5):
    """(PackedBatch, index, params, oracle arrays of the --faster model) of a scenario batch: one oracle run, shared and left unchanged."""
    pb, index = ps.batch_for(hap_len, read_len, mld)
    p = ps.params_for(mld, 0)
    return pb, index, p, oracle(p, pb)


def long_batch():
    """Ordinary windows beside the two smallest long shapes of the --faster model: one 767-bp haplotype, one 1,025-bp read."""
    from dindel_tgi_amd.batch import ReadRec, Window, pack
    rng = np.random.default_rng(767)
    S = ps.HAP_START
    h = [ps.rnd(rng, n) for n in (120, 767, 300, 90)]
    long_read = ps.mutate(rng, ps.seq_at(rng, h[2], -360, 1025), 0.02)
    ws = [Window(S, [h[0], h[0][:50] + h[0][53:]], ps.spread_reads(rng, h[0], 5, 36), hap_vars=[[(40, 44)], [(50, 50)]],
                 hap_var_flanks=[[(38, 46, 1)], [(48, 52, 2)]]),
          Window(S, [h[1], h[1][:400] + "ACGT" + h[1][400:]], ps.spread_reads(rng, h[1], 4, 50)),
          Window(S, [h[2]], ps.spread_reads(rng, h[2], 3, 36) + [ReadRec(long_read, [ps.Q30] * 1025, ps.MQ, S - 360)]),
          Window(S, [h[3]], ps.spread_reads(rng, h[3], 4, 30))]
    return pack(ws)


@functools.lru_cache(maxsize=None)
def long_scenario():
    pb = long_batch()
    p = ps.params_for(5, 0)
    return pb, p, oracle(p, pb)


def handmade_batch():
    """Hand-made pairs for the places the model can go wrong; -> (PackedBatch, {name: window}).  maxLengthDel 5 is meant."""
    from dindel_tgi_amd.batch import ReadRec, Window, pack
    rng = np.random.default_rng(20260)
    S = ps.HAP_START
    Q, Q20, MQ = ps.Q30, ps.Q20, ps.MQ
    hap = ps.rnd(rng, 80)
    names, ws = {}, []

    def add(name, window):
        names[name] = len(ws)
        ws.append(window)

    rd = lambda seq, start, q=Q, mq=MQ: ReadRec(seq, [q] * len(seq), mq, start)
    add("short reads", Window(S, [hap], [rd(hap[10:13], S + 10), rd(hap[10:14], S + 10), rd(hap[10:15], S + 10), rd("A", S + 3)]))       # L = 3 (NAN), 4 (one k-mer), 5, 1
    add("short haplotypes", Window(S, [hap[:6], hap[:7], hap[:5]], [rd(hap[:6], S), rd(hap[1:7], S + 1)]))                              # at maxLengthDel 5: hlen 5 is computed
    add("hlen 4 and 5", Window(S, ["ACGT", "ACGTA"], [rd("ACGT", S), rd("ACGTA", S), rd("CGTAC", S + 1)]))                               # HAPSIZE (4 < 5) / one hashed k-mer ... none
    add("hapsize", Window(S, ["AC", "ACG", hap], [rd(hap[5:41], S + 5)]))                                                                      # hlen < maxLengthDel
    junk = "".join("ACGT"[(i * 7 + i // 3) % 4] for i in range(36))
    add("junk", Window(S, ["A" * 60 + "C" * 20], [rd("GT" * 18, S + 10), rd("T" * 36, S + 20), rd(junk, S)]))                            # no k-mer hit: the sentinel alone
    tandem = "ACGT" * 30
    add("tandem", Window(S, [tandem, "AC" * 60, "A" * 100], [rd("ACGT" * 9, S + 40), rd("AC" * 20, S + 10), rd("A" * 36, S + 30), rd("CGTA" * 6 + "GG", S)]))
    add("left and right", Window(S, [hap], [rd(hap[:36], S - 200), rd(hap[40:76], S + 500), rd(hap[:36], S - 36), rd(hap[44:80], S + 81),
                                            rd(hap[:36], S - 35), rd(hap[44:80], S + 80)]))                                             # bMid = L - 1 / 0 and the edges
    iupac = hap[:20] + "NNRYacgtn" + hap[29:]
    add("alphabet", Window(S, [iupac, hap], [rd(iupac[10:46], S + 10), rd(hap[10:30] + "NnRy" + hap[34:46], S + 10), rd(hap[10:46].lower(), S + 10),
                                             rd("N" * 36, S + 10)]))
    mqs = [float(1.0 - 10 ** (-q / 10.0)) for q in (10, 39, 40, 44, 45, 46, 60)] + [1 - 1e-16, 0.5, 1e-16]
    add("mapping qualities", Window(S, [hap, hap[:40] + hap[43:]], [rd(hap[20:56], S + 20, Q20, mq) for mq in mqs] + [rd(ps.rnd(rng, 36), S + 20, Q, mq) for mq in mqs[:4]]))
    hv = [[(30, 33), (0, 2), (70, 79)], [(28, 30)]]
    hf = [[(28, 35, 1), (-3, 4, 2), (70, 85, 1)], [(26, 32, 2)]]
    add("variants", Window(S, [hap, hap[:30] + hap[33:]], ps.spread_reads(rng, hap, 6, 36) + [rd(hap[:40], S), rd(hap[40:], S + 40), rd(hap[20:23], S + 20)],
                           hap_vars=hv, hap_var_flanks=hf))
    return pack(ws), names


def result_struct(arrs, null=()):
    return ac.result_struct(arrs, null)
