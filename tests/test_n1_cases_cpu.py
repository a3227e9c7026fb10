"""The N1 case files (tests/_n1_cases.py) against the CPU references, without a GPU: the oracle's ddo_pair_sums is the
sequential Python loop bit for bit; the oracle meets the error bound B against a 200-bit evaluation (so B is a bound the
reference alone meets, not one fitted to the device); the exact-order cases do depend on the order; the directed map-pair
tables give the same answers in the host library (host/genotype.cpp) and in the Python restatement of the reference loop."""
import ctypes as C
import math

import numpy as np
import pytest

from dindel_tgi_amd import capi
from tests import _n1_cases as n1
from tests import _oracle
from tests.test_genotype_n1 import host_pair_posteriors, py_pair_posteriors

ALL_CASES = [(s, k) for s in n1.SHAPES for k in n1.CONTENTS]


def oracle_sums(pb, ll, n_slots):
    b = pb.ctypes_batch()
    out = np.full(max(n_slots, 1), n1.SENTINEL)
    lp = np.ascontiguousarray(ll if ll.size else np.zeros(1))
    assert _oracle.load().ddo_pair_sums(C.byref(b), lp.ctypes.data_as(capi.c_f64p), out.ctypes.data_as(capi.c_f64p)) == 0
    return out[:n_slots]


def test_shape_lists_cover_what_they_claim():
    ragged = [n1.SHAPES["ragged_%d" % k] for k in (1, 2, 3)]
    assert {w for s in ragged for w in s if w[0]} >= {(H, R) for H in n1.H_VALUES for R in n1.R_VALUES}
    for k, s in enumerate(ragged):
        H = [w[0] for w in s]
        assert sum(h * h for h in H) % 4 == k + 1                          # the last 4-wave block is partly empty
        assert H[0] == 0 and H[-1] == 0 and any(H[i] == 0 and H[i + 1] == 0 for i in range(1, len(H) - 2))
        assert {w[1] for w in s if w[0] >= 2} >= set(n1.R_VALUES)            # every R with a real pair
        assert sum(h * (h + 1) // 2 * r for h, r in s) < 2e5
    assert len(n1.SHAPES["single"]) == 1 and all(h == 0 for h, _ in n1.SHAPES["all_h0"])
    for name, s in n1.SHAPES.items():
        c = n1.case(name, "random")
        assert c["pb"].n_pairs == c["ll"].size == sum(h * r for h, r in s)
        H = np.diff(c["pb"].a["win_hap_off"]).astype(np.int64)
        assert np.array_equal(c["hh"], np.concatenate([[0], np.cumsum(H * H)]))


@pytest.mark.parametrize("shape,kind", ALL_CASES)
def test_oracle_is_the_sequential_loop(shape, kind):
    c = n1.case(shape, kind)
    got = oracle_sums(c["pb"], c["ll"], c["want"].size)
    nan = np.isnan(c["want"])
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(n1.bits(got[~nan]), n1.bits(c["want"][~nan]))
    if kind in ("one_side_minus_inf", "both_minus_inf") and c["want"].size:
        assert nan.any() and not nan.all()                                   # the NaN slots are some, not all
    else:
        assert np.isfinite(c["want"]).all()


def test_oracle_is_the_sequential_loop_on_the_exact_cases():
    shape, ll, slots = n1.exact_case()
    got = oracle_sums(n1.make_batch(shape), ll, int(n1.slot_offsets(shape)[-1]))
    want, _ = n1.sequential_reference(shape, ll)
    assert np.array_equal(n1.bits(got), n1.bits(want))
    assert got[n1.PROBE_SLOT] == n1.LOG_HALF
    for slot, row in slots:                                                  # glibc's exp / log are exact where they must be
        assert got[slot] == n1.seq_sum([n1.LOG_HALF + x for x in row.tolist()])


@pytest.mark.parametrize("R", n1.EXACT_R)
def test_exact_cases_depend_on_the_order(R):
    """Without this the bitwise comparison on the device proves nothing: reversed, wave-tree and exactly rounded sums of
    the same terms must all give other bits than the sequential sum."""
    assert n1.order_sensitive(R, n1.EXACT_SEEDS[R])
    for row in n1.exact_rows(R, n1.EXACT_SEEDS[R]):
        t = [n1.LOG_HALF + x for x in row.tolist()]
        other = n1.other_orders(t)
        assert set(other) == {"reversed", "chunk_tree", "fsum"}
        for name, v in other.items():
            assert v != n1.seq_sum(t), name
            assert abs(v - n1.seq_sum(t)) < 1e-12 * abs(v)                   # yet so close that rtol = 1e-12 cannot tell them apart


@pytest.mark.parametrize("shape,kind", [c for c in ALL_CASES if c[0] != "all_h0"])
def test_oracle_within_bound_of_200_bit_evaluation(shape, kind):
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp.clone()
    mp.prec = 200
    c = n1.case(shape, kind)
    got = oracle_sums(c["pb"], c["ll"], c["want"].size)
    half = mp.log(mp.mpf(0.5))
    memo = {}

    def term(a, b):                                                          # log(1/2) + log(e^a + e^b)
        hi, lo = max(a, b), min(a, b)
        if lo == -math.inf or hi - lo > 1e6:                                 # e^(lo - hi) < e^-1e6: far below 2^-200 of anything here
            return half + mp.mpf(hi)
        key = (hi, lo) if hi != lo else 0.0                                  # the difference itself is taken at 200 bits
        if key not in memo:
            memo[key] = mp.log1p(mp.exp(mp.mpf(lo) - mp.mpf(hi)))
        return half + mp.mpf(hi) + memo[key]

    ll, off, slot, worst = c["ll"].tolist(), 0, 0, 0.0
    for H, R in c["shape"]:
        rows = [ll[off + h * R:off + (h + 1) * R] for h in range(H)]
        for h1 in range(H):
            for h2 in range(H):
                if h2 >= h1 and math.isfinite(c["want"][slot]):
                    true = mp.fsum(term(a, b) for a, b in zip(rows[h1], rows[h2]))
                    err = float(abs(mp.mpf(float(got[slot])) - true))
                    assert err <= c["B"][slot], (slot, H, R, h1, h2, err, c["B"][slot])
                    if c["B"][slot]:
                        worst = max(worst, err / c["B"][slot])
                slot += 1
        off += H * R
    print("%s/%s: max |oracle - true| / B = %.3g" % (shape, kind, worst))


@pytest.mark.parametrize("sel", n1.SELECTIONS)
def test_map_tables_host_library_against_reference_loop(sel):
    seen = dict(none=0, some=0, tie_first=0)
    for H, ps, pr, f, nc in n1.map_windows(sel):
        if H == 0:
            continue
        want = py_pair_posteriors(H, ps, pr, f, nc)
        rc, post, pairs, vals = host_pair_posteriors(H, ps, pr, f.astype(np.int32), nc)
        if want[1] == [-1, -1]:
            assert rc == -1                                                  # no eligible indel pair: "Could not find indel allele"
            seen["none"] += 1
            continue
        assert rc == 0
        seen["some"] += 1
        assert np.array_equal(post, want[0], equal_nan=True)
        assert pairs.tolist() == want[1] + want[2]
        assert vals[0] == want[3] and vals[1] == want[4]
        assert vals[2] == want[5] or (math.isnan(vals[2]) and math.isnan(want[5]))
    assert seen["none"] > 0
    assert (seen["some"] > 0) == (sel not in ("all_filtered", "only_nocand"))


def test_map_tables_place_what_they_claim():
    """The tables' own preconditions, from the restatement: a placed maximum wins, a tie goes to the first of the two slots,
    and the interesting lanes and passes do occur."""
    placed = set()
    for sel in n1.SELECTIONS:
        for H in n1.MAP_H:
            f, nc = n1.selection(H, sel)
            ci, cn = n1.eligible(H, f, nc)
            for table in n1.TABLES:
                ps, pr = n1.map_table(H, table, f, nc)
                _, pi, pn, mi, mn, _ = py_pair_posteriors(H, ps, pr, f, nc)
                for cls, pair, top in ((ci, pi, -102.0), (cn, pn, -92.0)):
                    idx = pair[0] * H + pair[1] if pair[0] >= 0 else -1
                    if not cls or table == "all_minus_inf" or (table == "nan_winner" and len(cls) == 1):
                        assert idx == -1
                    elif table == "all_tie":
                        assert idx == cls[0] and (ps[cls] + pr[cls] == top).all()
                    elif table.startswith("max_"):
                        t = H * H - 1 if table == "max_last" else int(table[4:])
                        assert idx == n1._nearest(cls, t) and (idx == t or t not in cls)
                        placed.add((idx % 64, idx // 64))
                    elif table.startswith("tie_") and len(cls) > 1:
                        a, b = n1._tie_pair(cls, table == "tie_same_lane")
                        assert idx == a < b and ps[a] == ps[b]
                        placed.add((table, a % 64 == b % 64 and b == a + 64, a // 64 + 1 == b // 64 and a % 64 > b % 64))
                    elif table == "nan_winner":
                        assert math.isnan(ps[cls[0]]) and idx == cls[1]
    for lane_pass in ((0, 0), (63, 0), (0, 1), (1, 1), (63, 1), (0, 2), (528 % 64, 528 // 64)):
        assert lane_pass in placed, lane_pass
    assert ("tie_same_lane", True, False) in placed and ("tie_lane63_lane0", False, True) in placed
