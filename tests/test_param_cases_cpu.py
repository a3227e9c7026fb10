"""The parameter sets and the batch of tests/_param_cases.py reach what they are meant to reach — shown on the host alone: dd_build_tables
against a restatement of its formulas under every set, the threshold ladder and each set's claim on the oracle, the builds the GPU matrix
(tests/test_gpu_param_matrix.py) will launch from the plan's host arithmetic, and the values check_params refuses."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

from dindel_tgi_amd import capi
from tests import _oracle
from tests import _param_cases as pc
from tests import _path_scenarios as ps

NAN = float("nan")
INF = float("inf")
# table layout (hmm_kernel.h)
TC_LLL, TC_LFL, TC_II, TC_NI, TC_IN, TC_NN, TC_EDEF, TC_NDEF, TC_BQT, TC_HMQ, TC_FAST, TC_PINS = 0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 21
T_QUAL = 32
T_MAPQ = T_QUAL + 4 * 256
T_HP = T_MAPQ + 4 * 256
T_MAPQF = T_HP + 2 * 64
T_MAPQ2 = T_MAPQF + 2 * 256
T_END = T_MAPQ2 + 2 * 256
TABLE_QUALS = pc.BASE_QUALS + (1e-16, 0.999)
TABLE_MAPQS = pc.MAP_QUALS + (1.0, 1 - 1e-10, 0.99, 1 - 1e-5)         # (dd_build_tables takes 1.0; the compute entries refuse it)


def log(x):
    """C's log: -inf at 0 (math.log raises there)."""
    return -INF if x == 0.0 else math.log(x)


def log10(x):
    return -INF if x == 0.0 else math.log10(x)


def expected_tables(p, quals, mapqs):
    """dd_build_tables (batch_host.cpp) restated entry by entry: ObservationModelFB.cpp:226-234, 268-303, 1643-1703, Faster.cpp:117-124,
    300-352; python's math is the same libm."""
    out = [0.0] * capi.DD_TABLE_DOUBLES
    lIns = -.5
    lInsNoIns = log(p.pError)
    out[TC_LLL] = log(1.0 - p.pFirstgLO)
    out[TC_LFL] = log(p.pFirstgLO)
    out[TC_II] = lIns
    out[TC_NI] = log(1.0 - math.exp(lIns))
    out[TC_IN] = lInsNoIns
    out[TC_NN] = log(1 - p.pError)
    out[TC_EDEF] = log(1e-5)
    out[TC_NDEF] = log(1 - 1e-5)
    out[TC_BQT] = p.checkBaseQualThreshold
    for i, rq in enumerate(quals):
        pr = rq * (1.0 - p.pMut)
        out[T_QUAL + 4 * i:T_QUAL + 4 * i + 4] = [log(.25 + .75 * pr), log(.75 + 1e-10 - .75 * pr), log10(1.0 - rq), rq]

    def capped(mapQual, cap):
        mq = 1.0 - mapQual
        if -10.0 * log10(mq) > cap:
            mq = math.pow(10.0, -cap / 10.0)
        return mq

    for i, mapQual in [(-1, 1.0 - 1e-10)] + list(enumerate(mapqs)):
        mq = capped(mapQual, p.mapQualThreshold)
        dst = TC_HMQ if i < 0 else T_MAPQ + 4 * i
        for k in range(2):
            lp = lInsNoIns if k == 1 else log(1.0 - math.exp(lInsNoIns))
            out[dst + k] = log(mq) + lp + 0.0
            out[dst + 2 + k] = 0.0 + log(1.0 - mq) + lp
        dst = TC_PINS + 1 if i < 0 else T_MAPQ2 + 2 * i
        out[dst], out[dst + 1] = log(mq), log(1.0 - mq)
    out[TC_PINS] = log(1.0 - math.exp(lInsNoIns))
    out[TC_FAST:TC_FAST + 5] = [log(1.0 - p.pError), log(p.pError), log(1 - math.exp(-0.25)), log(1.0 - 1e-10), log(1e-10)]
    for i, mapQual in enumerate(mapqs):
        mq = capped(mapQual, p.capMapQualFast)
        out[T_MAPQF + 2 * i], out[T_MAPQF + 2 * i + 1] = log(1.0 - mq), log(mq)
    base = [2.9e-5] * 4 + [4.3e-5, 1.1e-4, 2.4e-4, 5.7e-4, 1.0e-3, 1.4e-3]
    for ln in range(64):
        n = max(ln, 1)
        pbe = (base[n - 1] if n <= 10 else base[9] + 4.3e-4 * float(n - 10)) * float(n)
        pbe = min(pbe, 0.99)
        out[T_HP + 2 * ln], out[T_HP + 2 * ln + 1] = log(pbe), log(1.0 - pbe)
    return np.asarray(out, np.float64)


def build_tables(lib, p, quals=TABLE_QUALS, mapqs=TABLE_MAPQS):
    q, m = np.asarray(quals, np.float64), np.asarray(mapqs, np.float64)
    out = np.full(capi.DD_TABLE_DOUBLES, 7.0)
    n = lib.dd_build_tables(C.byref(p), q.ctypes.data_as(capi.c_f64p), len(q), m.ctypes.data_as(capi.c_f64p), len(m), out.ctypes.data_as(capi.c_f64p))
    return n, out


@pytest.mark.parametrize("name", ["cli_defaults", "struct_defaults"] + list(pc.PARAM_SETS))
def test_tables_equal_the_restated_formulas_bit_for_bit(lib, name):
    for mld in (5, 15):
        p = {"cli_defaults": capi.params_cli_defaults, "struct_defaults": capi.params_struct_defaults}[name]() if name.endswith("defaults") else pc.params_for(name, mld)
        n, got = build_tables(lib, p)
        assert n == T_END, capi.last_error()
        want = expected_tables(p, TABLE_QUALS, TABLE_MAPQS)
        bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
        assert bad.size == 0, (name, bad[:8], got[bad[:8]], want[bad[:8]])
        assert not np.isnan(got).any(), (name, np.nonzero(np.isnan(got))[0])


def test_sets_put_the_extreme_constants_where_their_comments_say(lib):
    def table(name):
        return build_tables(lib, pc.params_for(name, 5))[1]
    t = table("tie")
    q1 = TABLE_QUALS.index(1.0)
    assert t[T_QUAL + 4 * q1] == math.log(.5) and t[T_QUAL + 4 * q1 + 1] == math.log(.5 + 1e-10) and t[T_QUAL + 4 * q1 + 2] == -INF
    assert 0 < t[T_QUAL + 4 * q1 + 1] - t[T_QUAL + 4 * q1] < 2.1e-10 and t[TC_BQT] == 0.0
    t = table("mismatch_wins")
    assert all(t[T_QUAL + 4 * i] == math.log(.25) and t[T_QUAL + 4 * i + 1] == math.log(.75 + 1e-10) for i in range(len(TABLE_QUALS)))
    t = table("exact")
    assert t[T_QUAL + 4 * q1] == 0.0 and t[T_QUAL + 4 * q1 + 1] == math.log(.75 + 1e-10 - .75) and -23.03 < t[T_QUAL + 4 * q1 + 1] < -23.02
    t = table("perror_tiny")
    assert t[TC_NN] == 0.0 and t[TC_IN] < -690 and t[TC_PINS] == 0.0
    t = table("perror_big")
    assert t[TC_IN] > t[TC_NN] and t[TC_HMQ + 3] > t[TC_HMQ + 2]
    assert table("lo_leaky")[TC_LFL] < -115 and table("lo_leaky")[TC_LLL] == 0.0
    assert -37 < table("lo_sticky")[TC_LLL] < -36.7
    t = table("mapq_cap_zero")
    assert t[TC_HMQ + 2] == -INF and t[TC_HMQ + 3] == -INF and all(t[T_MAPQ + 4 * i + 2] == -INF and t[T_MAPQF + 2 * i] == -INF for i in range(len(TABLE_MAPQS)))
    t = table("mapq_cap_high")
    m1 = TABLE_MAPQS.index(1.0)
    assert -231 < t[T_MAPQ + 4 * m1] < -230 and -231 < t[T_MAPQF + 2 * m1 + 1] < -230
    assert table("lo_never")[TC_LFL] == -INF and table("lo_always")[TC_LLL] == -INF


# ---- the oracle under the sets ----
@functools.lru_cache(maxsize=None)
def batch(hl, mld):
    return pc.batch_for(hl, mld)


@functools.lru_cache(maxsize=None)
def oracle(name, hl, mld, first_only=False):
    p = pc.default_params(mld) if name == "defaults" else pc.params_for(name, mld)
    return _oracle.batch(p, batch(hl, mld), nthreads=16, first_window=0, n_win=1 if first_only else -1)


def bmid_of(read, hap_len):
    """ObservationModelFB::Init's bMid of a mapped read that overlaps the haplotype (:35-102)."""
    start, L = read.start, len(read.seq)
    ol0, ol1 = max(ps.HAP_START, start), min(ps.HAP_START + hap_len, start + L - 1)
    assert ol0 <= ol1 and not read.unmapped
    return (ol1 - ol0) // 2 + ol0 - start


def half_wave_units(reads, hap_len, lo, hi):
    """The pairs of reads a G = 2 wavefront takes (hmm_kernel.hip, the ordering of a chunk): the reads of the launch's length class [lo, hi]
    by key = length bucket << 11 | bMid (descending in odd buckets), ties by index; two consecutive ranks per wavefront."""
    assert len(reads) <= 256
    keyed = []
    for i, r in enumerate(reads):
        L = len(r.seq)
        if lo <= L <= hi:
            bucket = (L - 1) >> 3
            if r.unmapped or r.start > ps.HAP_START + hap_len or r.start + L - 1 < ps.HAP_START:
                bm = L // 2
            else:
                bm = min(max(bmid_of(r, hap_len), 0), L - 1)
            keyed.append(((bucket << 11) | (1023 - bm if bucket & 1 else bm), i))
    order = [i for _k, i in sorted(keyed)]
    return [tuple(order[j:j + 2]) for j in range(0, len(order) - 1, 2)]


@pytest.mark.parametrize("mld", pc.MLDS)
def test_ladder_straddles_the_bound_of_the_speculative_pass(lib, mld):
    """Under `tie` the ladder at mapping quality 0.9999 has computed pairs on both sides of ll = -99 on the first haplotype, at every
    haplotype length of the matrix; ll falls strictly with the read's length; and in the half-wave classes one wavefront holds a pair from
    each side."""
    for hl in ps.hap_lengths(mld):
        pb = batch(hl, mld)
        want = oracle("tie", hl, mld, True)
        pairs = [pc.pair_of(pb, 0, 0, r) for r in pc.LADDER]
        ll, st = want["ll"][pairs], want["status"][pairs]
        assert (st == capi.DD_PAIR_OK).all(), (hl, st)
        assert (np.diff(ll) < 0).all(), (hl, ll)
        assert (ll > -99).any() and (ll < -99).any(), (hl, ll)
        above = max(n for n, v in zip(pc.LADDER_LENS, ll) if v > -99)
        print("ladder mld %d haplotype %d bp: ll > -99 up to %d bp (%.4f), < -99 from %d bp (%.4f)" % (mld, hl, above, ll[pc.LADDER_LENS.index(above)], above + 1, ll[pc.LADDER_LENS.index(above) + 1]))
        G = next(c[1] for c in capi.HAP_CLASSES if hl <= c[0])
        if G == 2 and mld <= 11:                                       # (the D = 32 build has whole wavefronts only)
            p = pc.params_for("tie", mld)
            cls = int(np.searchsorted(capi.HAP_CLASS_BOUNDS, hl))
            mine = [b for b in ps.planned_builds(lib, p, pb) if b[4] == cls and b[5] >= above + 1]
            assert mine and all(b[3] == 2 for b in mine), (hl, mine)
            hi = min(b[5] for b in mine)
            lo = max([b[5] + 1 for b in ps.planned_builds(lib, p, pb) if b[4] == cls and b[5] < hi] or [1])
            assert lo <= above, (hl, lo, hi)                           # both lengths in one launch
            reads = pc.case_windows(hl, mld, np.random.default_rng(pc.seed_of(hl, mld)))[0].reads
            units = half_wave_units(reads, hl, lo, hi)
            all_ll = want["ll"]
            split = [(a, b) for a, b in units if (all_ll[pc.pair_of(pb, 0, 0, a)] > -99) != (all_ll[pc.pair_of(pb, 0, 0, b)] > -99)]
            assert split, (hl, units)
            print("  half-wave class: wavefront of reads %s (%d / %d bp) has ll %.4f and %.4f" % (split[0], len(reads[split[0][0]].seq), len(reads[split[0][1]].seq),
                  all_ll[pc.pair_of(pb, 0, 0, split[0][0])], all_ll[pc.pair_of(pb, 0, 0, split[0][1])]))


CLAIM_POINTS = [(5, 30), (10, 126), (11, 127), (15, 574), (5, 766)]


@pytest.mark.parametrize("mld,hl", CLAIM_POINTS)
def test_sets_do_what_they_claim(mld, hl):
    pb = batch(hl, mld)
    n = pb.n_pairs
    dflt = oracle("defaults", hl, mld)
    for name in pc.PARAM_SETS:
        w = oracle(name, hl, mld)
        assert (w["status"][:n] == capi.DD_PAIR_OK).all(), name
        assert not any(np.isnan(w[k][:n]).any() for k in ("ll", "llOn", "llOff", "mLogBQ")), name
        assert (w["ll"][:n] != dflt["ll"][:n]).any(), name                 # a set that changes nothing tests nothing
    w = oracle("mapq_cap_zero", hl, mld)
    assert (w["offHap"][:n] == 1).all() and np.isneginf(w["llOn"][:n]).all()
    w = oracle("mismatch_wins", hl, mld)
    inside = [pc.pair_of(pb, 0, 0, pc.ROLE[(L, "inside")]) for L in pc.ORDINARY_LENS if L <= hl]
    assert inside or hl < min(pc.ORDINARY_LENS)
    assert (w["numMismatch"][inside] > 0).all() and (dflt["numMismatch"][inside] == 0).all(), (w["numMismatch"][inside], dflt["numMismatch"][inside])
    w = oracle("perror_big", hl, mld)
    assert ((w["numIndels"][:n] > 0) & (dflt["numIndels"][:n] == 0)).any()
    assert (oracle("exact", hl, mld)["nBQT"][:n] != oracle("tie", hl, mld)["nBQT"][:n]).any()
    for name in ("lo_sticky", "lo_always"):
        w = oracle(name, hl, mld)
        assert (w["hpos"][:pb.hpos_len] != dflt["hpos"][:pb.hpos_len]).any(), name


@pytest.mark.parametrize("mld,hl", [(5, 511), (15, 574), (10, 766)])
def test_lo_leaky_moves_the_path_of_the_overhanging_read_that_can_pay_for_leaving_lo(mld, hl):
    """pFirstgLO decides a path only where bMid is off the haplotype and enough matching bases follow (_param_cases.LO_SWITCH_MIN_HAP): the
    read that hangs 400 and more bases over the left end enters the haplotype under the defaults and stays in LO under lo_leaky and
    lo_never."""
    assert hl >= pc.LO_SWITCH_MIN_HAP
    pb = batch(hl, mld)
    pair = pc.pair_of(pb, 0, 0, pc.ROLE["lo_switch"])
    d = pc.hpos_of(pb, oracle("defaults", hl, mld), pair)
    assert (d >= 0).sum() >= 440 and d[0] == capi.DD_HPOS_LO
    for name in ("lo_leaky", "lo_never"):
        w = pc.hpos_of(pb, oracle(name, hl, mld), pair)
        assert (w == capi.DD_HPOS_LO).all() and (w != d).any(), name


def test_batch_is_small_and_a_function_of_its_point():
    for hl, mld in ((30, 5), (127, 11), (574, 15)):
        a, b = pc.batch_for(hl, mld), pc.batch_for(hl, mld)
        assert all(np.array_equal(a.a[k], b.a[k]) for k in a.a)
        ws = pc.case_windows(hl, mld, np.random.default_rng(pc.seed_of(hl, mld)))
        assert len(ws) == 2 and all(len(w.haps) == 3 and 25 <= len(w.reads) <= 45 for w in ws)
        assert max(len(h) for w in ws for h in w.haps) == hl and min(len(h) for w in ws for h in w.haps) > mld
        rl = [len(r.seq) for r in ws[0].reads[:2 * pc.N_LADDER]]
        assert rl == list(pc.LADDER_LENS) * 2                                                # adjacent lengths adjacent in the read order
        assert all(q == 1.0 for r in ws[0].reads[:2 * pc.N_LADDER] for q in r.qual)
        assert set(a.a["qual_table"].tolist()) >= set(pc.BASE_QUALS) and set(a.a["mapq_table"].tolist()) >= set(pc.MAP_QUALS)
        assert (a.a["read_flags"] & 1).sum() == 2 and a.var_cov_len > 0


def test_matrix_plans_every_build_the_plan_can_select(lib, monkeypatch):
    """The (K, Dt, gbt, G) planned over MLDS x hap_lengths under DD_FORCE_GBT unset, 0 and 1 hold every build dd_plan_info can return for
    those maxLengthDel with reads of 1 .. 146 bp (the enumeration of test_gpu_path_matrix's last test, at those read lengths)."""
    assert planned_union(lib, monkeypatch) >= pc.selectable(lib)
    print("parameter matrix: %d builds planned, %d selectable with reads of 1 .. %d bp" % (len(planned_union(lib, monkeypatch)), len(pc.selectable(lib)), max(pc.LADDER_LENS)))


def planned_union(lib, monkeypatch):
    reached = set()
    for gbt in (None, "0", "1"):
        if gbt is None:
            monkeypatch.delenv("DD_FORCE_GBT", raising=False)
        else:
            monkeypatch.setenv("DD_FORCE_GBT", gbt)
        for mld in pc.MLDS:
            for hl in ps.hap_lengths(mld):
                reached |= {b[:4] for b in ps.planned_builds(lib, pc.default_params(mld), batch(hl, mld))}
    monkeypatch.delenv("DD_FORCE_GBT", raising=False)
    return reached


# ---- what check_params refuses ----
REJECTED = [("pError", NAN), ("pError", 0.0), ("pError", 1.0), ("pMut", NAN), ("pMut", -1e-300), ("pMut", 1.0000000000000002), ("pMut", INF),
            ("pFirstgLO", NAN), ("pFirstgLO", -1e-300), ("pFirstgLO", 1.0000000000000002), ("mapQualThreshold", NAN), ("mapQualThreshold", -1e-300),
            ("mapQualThreshold", -INF), ("capMapQualFast", NAN), ("capMapQualFast", -0.5), ("checkBaseQualThreshold", NAN)]


@pytest.mark.parametrize("field,value", REJECTED, ids=["%s=%r" % r for r in REJECTED])
def test_invalid_parameters_are_refused_by_name(lib, field, value):
    """Each of these would put a NaN into the tables (the kernels' dmax() is defined for non-NaN doubles only)."""
    p = capi.params_cli_defaults()
    setattr(p, field, value)
    n, out = build_tables(lib, p)
    assert n == capi.DD_ERR_INVALID and field in capi.last_error(), (n, capi.last_error())
    assert (out == 7.0).all()                                             # nothing written
    from dindel_tgi_amd.batch import alloc_result
    pb = batch(30, 5)
    _arrs, res = alloc_result(pb)
    b = pb.ctypes_batch()
    for fn in (lib.dd_compute_likelihoods, lib.dd_compute_likelihoods_faster):       # validation comes before any device work
        assert fn(C.byref(p), C.byref(b), C.byref(res), 0) == capi.DD_ERR_INVALID and field in capi.last_error()


def test_edge_values_are_accepted(lib):
    for field, value in (("pMut", 0.0), ("pMut", 1.0), ("pFirstgLO", 0.0), ("pFirstgLO", 1.0), ("mapQualThreshold", 0.0), ("mapQualThreshold", INF),
                         ("capMapQualFast", 0.0), ("checkBaseQualThreshold", -INF), ("checkBaseQualThreshold", INF), ("pError", 5e-324)):
        p = capi.params_cli_defaults()
        setattr(p, field, value)
        n, out = build_tables(lib, p)
        assert n == T_END and not np.isnan(out).any(), (field, value, capi.last_error())
