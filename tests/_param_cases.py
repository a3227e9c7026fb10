"""Model parameters away from the two default sets, and one small batch to run under them (helper; no tests in here).

dd_build_tables turns pError, pMut, pFirstgLO, mapQualThreshold, capMapQualFast and checkBaseQualThreshold into the constants the four
likelihood kernels read (batch_host.cpp).  PARAM_SETS moves each of them to where the device code takes another turn; case_windows is a
batch small enough to run under every set on every selectable build.  tests/test_param_cases_cpu.py shows on the oracle that each set
does what its comment says; tests/test_gpu_param_matrix.py runs them on the device.

The threshold ladder: under `tie` every alignment of a read of base quality 1.0 costs log 0.5 per base (a match log .5, a mismatch
log(.5 + 1e-10)), so the best log-likelihood is a function of the read's length alone and crosses -99.0 — the bound below which
dd_hmm_kernel redoes its left-to-middle pass with the RO chain (hmm_kernel.hip, `for (int pass = 0; pass < 2; pass++)`) — between 142 and
143 bp.  Reads of LADDER_LENS put pairs on both sides of the bound into one launch and, on the half-wave builds, into one wavefront."""
import collections

import numpy as np

from dindel_tgi_amd import capi
from dindel_tgi_amd.batch import ReadRec, Window, pack, phred_to_prob
from tests import _path_scenarios as ps

PARAM_SETS = collections.OrderedDict([
    # match and mismatch emissions 2e-10 apart at quality 1.0: the -99 bound of the speculative pass inside the ladder, the oracle's tie
    # rules at every step, slice_argmax's count-one shortcut falls back to the replay; nBQT counts every base (quality > 0.0)
    ("tie", dict(pMut=2 / 3, checkBaseQualThreshold=0.0, padCover=0, maxMismatch=0)),
    # a match costs log .25, a mismatch log .75: the mismatch counters and var_fcov on reads that equal the haplotype; no base passes > 1.0
    ("mismatch_wins", dict(pMut=1.0, checkBaseQualThreshold=1.0, padCover=7, maxMismatch=5)),
    # quality 1.0: a mismatch costs log 1e-10 and the mLogBQ term is log10(0); the strict `>` of the TC_BQT compare at quality 0.5
    ("exact", dict(pMut=0.0, checkBaseQualThreshold=0.5)),
    # TC_NN == 0.0 exactly, TC_IN = -690: no inserted state survives a sweep
    ("perror_tiny", dict(pError=1e-300)),
    # log(pError) > log(1 - pError): the inserted-state prior and the NI transition beat the on-diagonal ones
    ("perror_big", dict(pError=0.9)),
    # TC_LFL = -115, below the RO prior of -100: leaving LO costs more than staying off the haplotype
    ("lo_leaky", dict(pFirstgLO=1e-50)),
    # TC_LLL = -36.7 per LO base: an overhanging read pays for every base left of the haplotype
    ("lo_sticky", dict(pFirstgLO=0.9999999999999999)),
    # on-haplotype prior -inf for every read, the HMQ prior included: -inf through both sweeps and the --faster model's on-haplotype term
    ("mapq_cap_zero", dict(mapQualThreshold=0.0, capMapQualFast=0.0)),
    # no cap in effect: a mapping quality of 1 - 1e-16 keeps its off-haplotype prior of -36.7 (capped: -23, --faster -10.4).  The -230 of a
    # mapping quality of exactly 1.0, below RO's -100, exists in dd_build_tables only (tests/test_param_cases_cpu.py): the compute entries
    # refuse a mapping quality outside [0,1) (host_path.cpp)
    ("mapq_cap_high", dict(mapQualThreshold=1000.0, capMapQualFast=1000.0)),
    # TC_LFL = -inf: no path leaves LO;  TC_LLL = -inf: no path stays in it
    ("lo_never", dict(pFirstgLO=0.0)),
    ("lo_always", dict(pFirstgLO=1.0)),
])

MLDS = (5, 10, 11, 15)                    # the D = 6, 11, 12 and 32 builds: the maxLengthDel values of _path_scenarios.GRID
LADDER_LENS = tuple(range(136, 147))      # both sides of the -99 bound under `tie` (142 / 143 bp)
LADDER_MQ, LADDER_LOW_MQ = 0.9999, 0.5
BASE_QUALS = (0.0, 0.25, 0.5, 0.949999999, 0.95, 0.950000001) + tuple(float(v) for v in phred_to_prob([2, 20, 40])) + (1 - 1e-10, 1.0)
MAP_QUALS = (0.0, 1e-16, 0.5, 0.9999, 1 - 1e-16)           # (1 - 1e-16 is the largest double below 1.0, the largest the library takes)
ORDINARY_LENS = (36, 100)
PLACES = ("inside", "left", "right", "far_left", "far_right", "beyond")
OVERHANGING = ("left", "right", "far_left", "far_right")

# read indices within the first window (the order case_windows builds them in)
N_LADDER = len(LADDER_LENS)
LADDER = range(0, N_LADDER)                                   # mapping quality 0.9999, lengths ascending
LADDER_LOW = range(N_LADDER, 2 * N_LADDER)                    # the same reads at mapping quality 0.5
ORDINARY0 = 2 * N_LADDER
ROLE = {(L, place): ORDINARY0 + len(PLACES) * i + j for i, L in enumerate(ORDINARY_LENS) for j, place in enumerate(PLACES)}
N_PLACED = len(ORDINARY_LENS) * len(PLACES)
ROLE.update(junk=ORDINARY0 + N_PLACED, deletion=ORDINARY0 + N_PLACED + 1, unmapped=ORDINARY0 + N_PLACED + 2)
N_READS0 = ORDINARY0 + N_PLACED + 3
# pFirstgLO acts only where bMid is off the haplotype: in passMessageTwoInc's state 0 and passMessageTwoDec's RO state
# (ObservationModelFB.cpp:1715-1829).  There a base in LO costs log(1 - pFirstgLO) + log(1 - pError) = -0.0105 under the defaults where a
# matching base on the haplotype costs twice log(1 - 2.9e-5): entering the haplotype (log pFirstgLO = -4.6) pays only after some 440
# matching bases.  So the haplotypes of LO_SWITCH_MIN_HAP bp and more get one read of DD_MAX_READ_LEN bp (ROLE["lo_switch"], the first
# window's last read): random bases, then the haplotype's start, mapped as if it began at the haplotype's start.  Its bMid lies in the
# random part; under the defaults the path right of bMid enters the haplotype, under lo_leaky it stays in LO.
LO_SWITCH_MIN_HAP = 500
ROLE["lo_switch"] = N_READS0


def params_for(name, mld, **kw):
    """PARAM_SETS[name] on top of the command line's defaults, at maxLengthDel mld."""
    d = capi.params_cli_defaults().as_dict()
    d.update(PARAM_SETS[name], maxLengthDel=mld, **kw)
    return capi.dd_params.from_dict(d)


def default_params(mld):
    d = capi.params_cli_defaults().as_dict()
    d.update(maxLengthDel=mld)
    return capi.dd_params.from_dict(d)


def ladder_read(rng, hap, n, mq):
    off = (len(hap) - n) // 2                                  # (negative: the read hangs over both ends)
    return ReadRec(ps.seq_at(rng, hap, off, n), [1.0] * n, mq, ps.HAP_START + off)


def ordinary_reads(rng, hap, start=0):
    """ORDINARY_LENS x PLACES, one junk read, one read with a 2-bp deletion, one read flagged unmapped: base qualities drawn from
    BASE_QUALS per base (the reads inside the haplotype equal it: they carry no substitution), mapping qualities MAP_QUALS in turn from
    `start`."""
    Hs = len(hap)
    reads = []

    def add(seq, off, **kw):
        q = [float(v) for v in rng.choice(BASE_QUALS, len(seq))]
        reads.append(ReadRec(seq, q, MAP_QUALS[(start + len(reads)) % len(MAP_QUALS)], (ps.HAP_START + off) & 0xFFFFFFFF, **kw))

    for L in ORDINARY_LENS:
        ov = L // 3
        far = 2 * L // 3
        # PLACES (inside: over both ends of a shorter haplotype).  far_left / far_right hang over by two thirds while their mapped start says
        # they lie at the haplotype's end: bMid, the middle of the mapped overlap, is then a base the true alignment has in LO / RO
        for off, at in (((Hs - L) // 2, None), (-ov, None), (Hs - L + ov, None), (-far, 0), (Hs - L + far, max(0, Hs - L)), (Hs + 5, None)):
            add(ps.seq_at(rng, hap, off, L), off if at is None else at)
    add(ps.rnd(rng, 100), max(0, (Hs - 100) // 2))
    Lr = max(4, min(100, Hs - 2))
    left = Lr // 2
    c = left + max(0, (Hs - 2 - Lr) // 2)
    add(hap[c - left:c] + hap[c + 2:c + 2 + Lr - left], c - left)
    L = min(76, Hs)
    add(ps.seq_at(rng, hap, (Hs - L) // 2, L), (Hs - L) // 2, unmapped=True)
    return reads


def case_windows(hap_len, mld, rng, extra_read=None):
    """Two windows, the same for every parameter set.
    The first: a random haplotype of hap_len bp, that haplotype without 2 bp and with 3 bp inserted (variants() flanks attached), under
    the ladder at mapping quality 0.9999 (reads LADDER), the ladder at 0.5 (LADDER_LOW), the ordinary reads (ROLE) and, from
    LO_SWITCH_MIN_HAP bp, the lo_switch read.
    The second: a haplotype around an AC repeat, as in _path_scenarios.ties_windows, under repeat reads, the ladder and ordinary reads.
    extra_read(window) -> ReadRec: one more read at the end of each window (the long-window tests force DD_WIN_LONG with it)."""
    hap = ps.rnd(rng, hap_len)
    m = hap_len // 2
    haps = [hap, ps.shorter(hap, 2, m, mld), (hap[:m] + ps.rnd(rng, 3) + hap[m:])[:hap_len]]      # (cut to hap_len: it stays the batch's longest)
    reads = [ladder_read(rng, hap, n, LADDER_MQ) for n in LADDER_LENS]
    reads += [ReadRec(r.seq, list(r.qual), LADDER_LOW_MQ, r.start) for r in reads]
    reads += ordinary_reads(rng, hap)
    assert len(reads) == N_READS0
    if hap_len >= LO_SWITCH_MIN_HAP:
        n = min(hap_len - 6, capi.DD_MAX_READ_LEN - (hap_len // 2 + 40))
        reads.append(ReadRec(ps.rnd(rng, capi.DD_MAX_READ_LEN - n) + hap[:n], [ps.Q30] * capi.DD_MAX_READ_LEN, LADDER_MQ, ps.HAP_START))
    hv, hf = ps.variants(haps)
    first = Window(ps.HAP_START, haps, reads, hap_vars=hv, hap_var_flanks=hf)

    unit = "AC"
    rep_len = max(12, min(60, hap_len // 2))
    n_rep = rep_len // len(unit)
    left = (hap_len - n_rep * len(unit)) // 2
    rhap = ps.rnd(rng, left) + unit * n_rep + ps.rnd(rng, hap_len - left - n_rep * len(unit))
    rep = unit * (n_rep + 80)
    rhaps = [rhap, ps.shorter(rhap, len(unit), left, mld), ps.rnd(rng, hap_len)]
    rreads = [ReadRec(rep[:k], [1.0] * k, LADDER_MQ, ps.HAP_START + left) for k in sorted({max(2, rep_len // 5), max(4, rep_len // 2)})]
    k = n_rep * len(unit) + 2 * len(unit) + 4                                                 # longer than the repeat
    rreads.append(ReadRec(rep[:k], [ps.Q20] * k, float(phred_to_prob([20])[0]), ps.HAP_START + left - len(unit) - 2))
    rreads.append(ReadRec(rep[:143], [1.0] * 143, LADDER_MQ, ps.HAP_START + left - 40))       # nothing but the repeat, at the bound
    rreads += [ladder_read(rng, rhap, n, LADDER_MQ) for n in LADDER_LENS]
    rreads += ordinary_reads(rng, rhap, start=3)
    hv, hf = ps.variants(rhaps)
    second = Window(ps.HAP_START, rhaps, rreads, hap_vars=hv, hap_var_flanks=hf)
    ws = [first, second]
    if extra_read is not None:
        for w in ws:
            w.reads.append(extra_read(w))
    return ws


def seed_of(hap_len, mld):
    return 7000003 * mld + hap_len


def batch_for(hap_len, mld):
    """-> PackedBatch of the point; a function of (hap_len, mld)."""
    return pack(case_windows(hap_len, mld, np.random.default_rng(seed_of(hap_len, mld))))


def long_batch_for(hap_len, mld):
    """The same windows with one read of LONG_FORCE_LEN bp each, so that the screen classes them DD_WIN_LONG whatever their length."""
    side = np.random.default_rng(seed_of(hap_len, mld) + 7919)

    def force(window):
        src = window.haps[0]
        off = (len(src) - ps.LONG_FORCE_LEN) // 2
        return ReadRec(ps.mutate(side, ps.seq_at(side, src, off, ps.LONG_FORCE_LEN), 0.02), [ps.Q30] * ps.LONG_FORCE_LEN, ps.MQ, ps.HAP_START + off)

    return pack(case_windows(hap_len, mld, np.random.default_rng(seed_of(hap_len, mld)), extra_read=force))


def pair_of(pb, window, hap, read):
    """Index of a pair in the result arrays (window-major, then haplotype, then read)."""
    R = int(pb.a["win_read_off"][window + 1] - pb.a["win_read_off"][window])
    return int(pb.win_pair_off[window]) + hap * R + read


def hpos_of(pb, arrs, pair):
    """The hpos slice of a pair."""
    elem = ps.element_pairs(pb)["hpos"][:pb.hpos_len]
    return arrs["hpos"][:pb.hpos_len][elem == pair]


def first_difference(got, want, pb):
    """None, or (array, element, pair) of the first difference in what assert_same compares and in the hpos of every computed pair."""
    d = ps.first_difference(got, want, pb, {})
    return None if d is None else d[:3]


def selectable(lib):
    """Every (K, Dt, gbt, G) dd_plan_info can return under the default environment for MLDS with reads of 1 .. 146 bp: the enumeration of
    tests/test_gpu_path_matrix.py's last test at the read lengths of case_windows' short reads."""
    import ctypes as C
    out = (C.c_int32 * 10)()
    can = set()
    for mld in MLDS:
        p = ps.params_for(mld, 0)
        for hl in sorted({1} | {h for b in capi.HAP_CLASS_BOUNDS for h in (b, b + 1) if h <= capi.DD_MAX_HAP_LEN}):
            for rl in range(1, max(LADDER_LENS) + 1):
                if lib.dd_plan_info(C.byref(p), hl, rl, 256, 50, 100, C.byref(out)) == 0:
                    can.add((out[0], out[1], out[2], out[8]))
    return can
