"""Directed cases for the N1 pair kernels (dd_pair_sum_kernel / dd_map_pair_kernel, csrc/genotype_kernel.hip): batches
whose only interesting property is their offsets, caller-made `ll` contents, the sequential reference, the error bound
B and the map-pair tables.  No GPU in here; tests/test_n1_cases_cpu.py checks these cases against the oracle and the
host library, tests/test_gpu_n1_matrix.py runs them on the device.

The error bound B (used instead of a flat rtol)
-----------------------------------------------
A slot is  S = sum_r t_r,  t_r = log(1/2) + (M + log(1 + exp(-|l1 - l2|))),  M = max(l1, l2) <= 0,  added in read order.
With u = 2^-53, to first order in u:

  * the recursive sum of R terms makes R - 1 rounded additions (0.0 + t_0 is exact); the classical bound is
    (R - 1) u sum_r |t_r|;
  * one term: e = exp(d), d <= 0, is documented to 1 ulp by HIP (glibc is tighter): an absolute error <= min(2 u e, u).
    x = 1 + e lies in [1, 2] and rounds with an absolute error <= u, so x is off by at most (min(2ue, u) + u) / (1 + e)
    <= 4u/3 relative, which is the absolute error it causes in log x.  log x lies in [0, ln 2], where 1 ulp is <= u.  So
    L = log(1 + e) carries <= 7u/3.  M + L rounds with <= u |M + L|; the constant log(1/2) is within 1 ulp = u; the last
    addition rounds with <= u |t_r|.  Because M <= 0 <= L <= ln 2 either |M + L| <= |M| <= |t_r|, giving
    7u/3 + u + 2u |t_r|, or 0 <= M + L <= ln 2 < 1, where a rounding is <= u/2, giving 7u/3 + u/2 + u + u |t_r|.
    Both are <= 2u |t_r| + 4u.

  B = (R - 1) u sum_r |t_r| + sum_r (2u |t_r| + 4u).

Every evaluation that keeps the read order and uses 1-ulp exp / log is within B of the true value, so two of them (the
device and the oracle) are within 2 B of each other.  B says nothing about another summation order; that is what the
exact-order cases are for.  The |t_r| used are the reference's own terms (the difference is second order).  B holds for
ll <= 0, which every case here keeps."""
import functools
import math

import numpy as np

from dindel_tgi_amd.batch import ReadRec, Window, pack

U = 2.0 ** -53
LOG_HALF = math.log(0.5)
SENTINEL = -1.2345678901234567e+123            # what outputs are pre-filled with; no case produces it
SENTINEL_I32 = 0x5A5A5A5A
HAP = "ACGTTGCAACGGTCATGCAT"
H_VALUES = (1, 2, 3, 5, 8, 9)
R_VALUES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)
EXACT_R = (63, 64, 65, 128, 129, 200)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def bits1(x):
    return int(np.array([x], np.float64).view(np.uint64)[0])


def make_batch(shape):
    """[(H, R)] per window -> PackedBatch: 20-bp haplotypes, 1- and 2-bp reads (only the offsets matter)."""
    ws = []
    for i, (H, R) in enumerate(shape):
        start = 1000 + 100 * i
        reads = [ReadRec(HAP[:1 + (r & 1)], [0.99] * (1 + (r & 1)), 0.99, start) for r in range(R)]
        ws.append(Window(start, [HAP] * H, reads))
    return pack(ws)


def _ragged(k):
    """Ragged list k = 0, 1, 2: every R of R_VALUES with two H of H_VALUES (the three lists together hold all 60 combinations),
    in shuffled order, windows without haplotypes first, twice in a row in the middle and last; n_slots = k + 1 (mod 4)."""
    rng = np.random.default_rng(100 + k)
    ws = []
    for ri, R in enumerate(R_VALUES):
        ws += [(H_VALUES[(ri + k) % 6], R), (H_VALUES[(ri + k + 3) % 6], R)]
    ws = [ws[i] for i in rng.permutation(len(ws))]
    need = (k + 1 - sum(H * H for H, _ in ws)) % 4
    for j in range(need):                                      # H = 1 adds one slot
        ws.insert(5 + 6 * j, (1, (2, 0, 1)[j]))
    mid = len(ws) // 2
    ws = [(0, 3)] + ws[:mid] + [(0, 0), (0, 64)] + ws[mid:] + [(0, 1)]
    assert sum(H * H for H, _ in ws) % 4 == k + 1
    return ws


SHAPES = {
    "ragged_1": _ragged(0),
    "ragged_2": _ragged(1),
    "ragged_3": _ragged(2),
    "single": [(3, 65)],
    "all_h0": [(0, 3), (0, 0), (0, 5)],
}
CONTENTS = ("random", "equal_rows", "hap_minus_1e300", "one_side_minus_inf", "both_minus_inf", "gap_below_underflow",
            "tiny_gap", "zeros")


def make_ll(shape, kind, seed=0):
    """The caller-made ll of a batch: per window H rows of R doubles at win_pair_off[w]."""
    rng = np.random.default_rng([seed, CONTENTS.index(kind)])
    out = []
    for H, R in shape:
        a = rng.uniform(-150.0, -5.0, (H, R))
        if kind == "equal_rows":
            a[:] = a[:1]
        elif kind == "hap_minus_1e300":
            a[1::2] = -1e300
        elif kind == "one_side_minus_inf":                     # the pair (1, 1) has it on both sides: NaN there, by the reference too
            a[1:2, ::3] = -math.inf
        elif kind == "both_minus_inf":                         # one read, haplotypes 0 and 1: NaN in (0,0), (0,1), (1,1) only
            a[:2, R // 2:R // 2 + 1] = -math.inf
        elif kind == "gap_below_underflow":
            a[1::2] = a[:1] - rng.uniform(750.0, 900.0, (len(a[1::2]), R))
        elif kind == "tiny_gap":
            a = -rng.uniform(1.0, 9.0, (1, R)) * 1e-16 - np.arange(H)[:, None] * 1e-17
        elif kind == "zeros":
            a[:] = 0.0
        out.append(np.ascontiguousarray(a, np.float64).reshape(-1))
    return np.concatenate(out) if out else np.zeros(0)


def add_logs(l1, l2):
    if l1 > l2:
        return l1 + math.log(1.0 + math.exp(l2 - l1))
    return l2 + math.log(1.0 + math.exp(l1 - l2))


def pair_terms(l1, l2, log5=LOG_HALF):
    return [log5 + add_logs(a, b) for a, b in zip(l1, l2)]


def seq_sum(terms):
    s = 0.0
    for t in terms:
        s += t
    return s


def bound(terms):
    a = sum(abs(t) for t in terms)
    return (len(terms) - 1) * U * a + 2.0 * U * a + 4.0 * U * len(terms) if terms else 0.0


def sequential_reference(shape, ll):
    """(sums, B) per slot: the loop of DInDel.cpp:3085-3091 in plain Python floats; lower triangle 0.0."""
    sums, B = [], []
    off = 0
    ll = ll.tolist()
    for H, R in shape:
        rows = [ll[off + h * R:off + (h + 1) * R] for h in range(H)]
        for h1 in range(H):
            for h2 in range(H):
                t = pair_terms(rows[h1], rows[h2]) if h2 >= h1 else []
                sums.append(seq_sum(t))
                B.append(bound(t))
        off += H * R
    return np.array(sums, np.float64), np.array(B, np.float64)


def slot_offsets(shape):
    return np.concatenate([[0], np.cumsum([H * H for H, _ in shape])]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def case(shape_name, kind):
    """dict(shape, pb, ll, want, B, hh) of one (shape list, ll contents) case; computed once, shared, never modified."""
    shape = SHAPES[shape_name]
    ll = make_ll(shape, kind)
    want, B = sequential_reference(shape, ll)
    for a in (ll, want, B):
        a.setflags(write=False)
    return dict(shape=shape, pb=make_batch(shape), ll=ll, want=want, B=B, hh=slot_offsets(shape))


# ---- exact-order cases -------------------------------------------------------------------------------------------------------
# One haplotype row is U(-150, -5), the other -1e300: exp(-1e300) == 0 and log(1.0) == 0 on any conforming libm, so a term is
# exactly log(1/2) + l[r] and the slot is a pure statement about the ORDER of R additions.
def chunk_tree_sum(terms):
    """The sum a wavefront butterfly makes: 64-wide chunks, each reduced by a xor tree (offsets 32 .. 1), lane 0 added on."""
    s = 0.0
    for c in range(0, len(terms), 64):
        v = list(terms[c:c + 64]) + [0.0] * (64 - len(terms[c:c + 64]))
        off = 32
        while off:
            v = [v[i] + v[i ^ off] for i in range(64)]
            off >>= 1
        s += v[0]
    return s


def other_orders(terms):
    return dict(reversed=seq_sum(terms[::-1]), chunk_tree=chunk_tree_sum(terms), fsum=math.fsum(terms))


EXACT_SEEDS = {63: 2, 64: 4, 65: 0, 128: 3, 129: 2, 200: 1}       # the first seeds for which order_sensitive() holds


def exact_rows(R, seed):
    rng = np.random.default_rng([7, R, seed])
    return rng.uniform(-150.0, -5.0, R), rng.uniform(-150.0, -5.0, R)


def order_sensitive(R, seed, log5=LOG_HALF):
    """Whether both exact pairs of the R window give other bits under each of the other orders."""
    for row in exact_rows(R, seed):
        t = [log5 + x for x in row.tolist()]
        if any(v == seq_sum(t) for v in other_orders(t).values()):
            return False
    return True


def exact_case():
    """Window 0 is the probe (H = 2, R = 1, ll = (0.0, -1e300): slot (0, 1) is 0.0 + (log(1/2) + 0.0), the device's own
    log(0.5)); window 1 + i has R = EXACT_R[i], H = 3 with rows (random, -1e300, random): pairs (0, 1) and (1, 2) are exact.
    Returns (shape, ll, [(slot, row)]) with row the random row whose terms the slot adds."""
    shape = [(2, 1)] + [(3, R) for R in EXACT_R]
    ll = [np.array([0.0, -1e300])]
    hh = slot_offsets(shape)
    slots = []
    for i, R in enumerate(EXACT_R):
        a, b = exact_rows(R, EXACT_SEEDS[R])
        ll.append(np.concatenate([a, np.full(R, -1e300), b]))
        slots += [(int(hh[1 + i]) + 1, a), (int(hh[1 + i]) + 5, b)]
    return shape, np.concatenate(ll), slots


PROBE_SLOT = 1


# ---- directed map-pair tables ------------------------------------------------------------------------------------------------
MAP_H = (1, 2, 8, 9, 12, 23)
SELECTIONS = ("mixed", "mixed_filtered", "all_filtered", "only_cand", "only_nocand", "one_unfiltered")
TABLES = ("distinct", "all_tie", "max_0", "max_63", "max_64", "max_65", "max_127", "max_128", "max_last", "tie_same_lane",
          "tie_lane63_lane0", "nan_winner", "all_minus_inf")


def selection(H, sel):
    """(filtered, ncand) of one window."""
    f = np.zeros(H, np.uint8)
    nc = (np.arange(H) % 3 != 0).astype(np.int32) * 2
    if sel == "mixed_filtered":
        f[1::5] = 1
    elif sel == "all_filtered":
        f[:] = 1
    elif sel == "only_cand":
        nc[:] = 1
    elif sel == "only_nocand":
        nc[:] = 0
    elif sel == "one_unfiltered":
        f[:] = 1
        f[H // 2] = 0
    return f, nc


def eligible(H, f, nc):
    """Row-major upper-triangle slots of unfiltered pairs: (with a candidate indel, without)."""
    ci, cn = [], []
    for h1 in range(H):
        for h2 in range(h1, H):
            if not f[h1] and not f[h2]:
                (ci if nc[h1] > 0 or nc[h2] > 0 else cn).append(h1 * H + h2)
    return ci, cn


def _nearest(slots, t):
    return min(slots, key=lambda s: (abs(s - t), s))


def _tie_pair(slots, same_lane):
    """a < b of one class: same lane in passes 0 and 1, or a on a higher lane of one pass and b on a lower lane of the
    next (nearest to 63 / 64); without a second pass any two slots."""
    S = set(slots)
    if same_lane:
        c = [(a, a + 64) for a in slots if a < 64 and a + 64 in S]
    else:
        c = [(a, b) for a in slots for b in slots if b // 64 == a // 64 + 1 and b % 64 < a % 64]
        c.sort(key=lambda p: (abs(p[0] - 63) + abs(p[1] - 64), p))
    if c:
        return c[0]
    return (slots[0], slots[-1]) if len(slots) > 1 else None


def map_table(H, table, f, nc):
    """(pair_sum, prior) of H * H doubles.  All values are small integers, so pair_sum + prior is exact and a tie is a tie.
    The background is distinct per slot and decreasing, lower-triangle and filtered slots included (they must be ignored:
    they hold the largest values of all)."""
    n = H * H
    ps = -500.0 - np.arange(n, dtype=np.float64)
    pr = np.full(n, -2.0)
    ci, cn = eligible(H, f, nc)
    skip = np.ones(n, bool)
    skip[ci + cn] = False
    ps[skip] = 1000.0                                          # never read, or read and discarded
    for cls, top in ((ci, -100.0), (cn, -90.0)):
        if not cls:
            continue
        if table == "all_tie":
            ps[cls] = top
        elif table.startswith("max_"):
            t = n - 1 if table == "max_last" else int(table[4:])
            ps[_nearest(cls, t)] = top
        elif table.startswith("tie_"):
            p = _tie_pair(cls, table == "tie_same_lane")
            if p:
                ps[list(p)] = top
        elif table == "nan_winner":                            # the background's winner is the first slot of the class
            ps[cls[0]] = math.nan
            if len(cls) > 2:
                ps[cls[-1]] = math.nan
        elif table == "all_minus_inf":
            ps[cls] = -math.inf
    if table == "all_minus_inf":
        ps[:] = -math.inf
    return ps, pr


def map_windows(sel):
    """One ragged launch for a selection class: [(H, pair_sum, prior, filtered, ncand)] with every table at every H of MAP_H
    in shuffled order, windows without haplotypes first, twice in a row in the middle and last; W is no multiple of 4."""
    rng = np.random.default_rng(SELECTIONS.index(sel))
    ws = []
    for H in MAP_H:
        f, nc = selection(H, sel)
        for table in TABLES:
            ws.append((H,) + map_table(H, table, f, nc) + (f, nc))
    ws = [ws[i] for i in rng.permutation(len(ws))]
    empty = (0, np.zeros(0), np.zeros(0), np.zeros(0, np.uint8), np.zeros(0, np.int32))
    mid = len(ws) // 2
    ws = [empty] + ws[:mid] + [empty, empty] + ws[mid:] + [empty]
    if len(ws) % 4 == 0:
        ws.append(empty)
    return ws
