"""Shared by the device-CIGAR tests: the host specification (ddh_get_cigar = dindel::getCIGAR) applied to a whole batch, a Python
restatement of the same walk that also says which branches it took, and the generated inputs (haplotype-to-reference maps, adversarial
alignments nobody's traceback would emit)."""
import ctypes as C

import numpy as np

from dindel_tgi_amd import capi
from dindel_tgi_amd.batch import PackedBatch, phred_to_prob
from tests import _host

M, I, D, S = 0, 1, 2, 4
INS, DEL, LO, RO = -1, -2, -3, -4
# ddh_get_cigar's negative returns -> per-pair status of the device (dd_cigar_result.status)
HOST_CODE_TO_STATUS = {-1: capi.DD_CIGAR_HAP_NOT_ALIGNED, -3: capi.DD_CIGAR_ERROR1, -4: capi.DD_CIGAR_ERROR2, -5: capi.DD_CIGAR_ERROR3,
                       -6: capi.DD_CIGAR_ERROR4, -7: capi.DD_CIGAR_IMPOSSIBLE}
# Every branch of host/cigar.cpp's walk.  "error1" is missing on purpose: the walk cannot reach it.  `here == INS` inside the aligned
# stretch means the step before had `next == INS`, which either threw or left op == CIG_INS (reference -> insertion sets it, "the
# insertion goes on" keeps it), and the first base of the stretch has a position; so `op != CIG_INS` never holds at that throw.
# "Read is not properly aligned!" and "Haplotype has not been aligned!" compare sizes the hook passes equal; the latter is the device's
# hap_aligned flag and is expected from the flag alone.
BRANCHES = {"all_clipped", "lead_clip", "trail_clip", "ins_goes_on", "ref_to_ins", "consecutive", "deletion", "ins_to_ref", "ins_then_del",
            "fall_through", "error2", "error3", "error4", "impossible", "next_not_after_here", "ins_next_not_after_anchor"}


def host_cigar(hap_ref, hpos_ref_codes):
    """ddh_get_cigar with refSeqStart 0: ([(op, len)], refPos) or the negative code of the string it threw."""
    lib = _host.load()
    hr = np.ascontiguousarray(hap_ref, np.int32)
    hp = np.ascontiguousarray(hpos_ref_codes, np.int16)
    out = np.zeros(4 * len(hp) + 8, np.int32)
    rp = C.c_int(0)
    n = lib.ddh_get_cigar(hr.ctypes.data_as(C.POINTER(C.c_int)), len(hr), hp.ctypes.data_as(C.POINTER(C.c_short)), len(hp), 0,
                          out.ctypes.data_as(C.POINTER(C.c_int)), len(out), C.byref(rp))
    if n < 0:
        return n
    return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)], rp.value


def walk(hap_ref, hpos):
    """The same walk in Python (host/cigar.cpp line by line) -> (host_cigar's result, set of BRANCHES taken)."""
    on = [hap_ref[h] if h >= 0 else h for h in hpos]
    n, took, cig = len(on), set(), []
    last = n - 1
    while last >= 0 and on[last] < 0:
        last -= 1
    if last < 0:
        return ([(S, n)], -1), {"all_clipped"}
    b = 0
    while on[b] < 0:
        b += 1
    if b > 0:
        cig.append((S, b)); took.add("lead_clip")
    anchor = ref_pos = on[b]
    op, ln = M, 1
    while b < last:
        here, nxt = on[b], on[b + 1]
        if nxt == INS:
            if here == INS:
                if op != I:
                    return -3, took
                ln += 1; took.add("ins_goes_on")
            elif here >= 0:
                if op != M:
                    return -4, took | {"error2"}
                cig.append((M, ln)); op, ln, anchor = I, 1, here; took.add("ref_to_ins")
            else:
                return -7, took | {"impossible"}
        elif here >= 0 and nxt >= 0 and nxt - here == 1:
            if op != M:
                return -5, took | {"error3"}
            ln += 1; anchor = nxt; took.add("consecutive")
        elif here >= 0 and nxt >= 0 and nxt - here > 1:
            if op != M:
                return -6, took | {"error4"}
            cig += [(M, ln), (D, nxt - here - 1)]; op, ln, anchor = M, 1, nxt; took.add("deletion")
        elif here == INS and nxt - anchor == 1:
            cig.append((I, ln)); op, ln, anchor = M, 1, nxt; took.add("ins_to_ref")
        elif here == INS and nxt - anchor > 1:
            cig += [(I, ln), (D, nxt - anchor - 1)]; op, ln, anchor = M, 1, nxt; took.add("ins_then_del")
        else:
            took.add("fall_through")
            if here >= 0 and nxt >= 0:
                took.add("next_not_after_here")
            if here == INS:
                took.add("ins_next_not_after_anchor")
        b += 1
    cig.append((op, ln))
    if n - 1 - last > 0:
        cig.append((S, n - 1 - last)); took.add("trail_clip")
    return (cig, ref_pos), took


def pair_hpos_slices(pb):
    """(pair index, haplotype, slice of the batch's hpos array) for every pair, in pair order."""
    a = pb.a
    rso = a["read_seq_off"].astype(np.int64)
    for w in range(pb.n_windows):
        h0, h1 = int(a["win_hap_off"][w]), int(a["win_hap_off"][w + 1])
        q0, q1 = int(a["win_read_off"][w]), int(a["win_read_off"][w + 1])
        SL = int(rso[q1] - rso[q0])
        for h in range(h1 - h0):
            for r in range(q1 - q0):
                s = int(pb.win_hpos_off[w]) + h * SL + int(rso[q0 + r] - rso[q0])
                yield int(pb.win_pair_off[w]) + h * (q1 - q0) + r, h0 + h, slice(s, s + int(rso[q0 + r + 1] - rso[q0 + r]))


def expected(pb, hpos, hap_ref_pos, hap_aligned, pair_status, ops_cap, fill):
    """What dd_cigars_device must leave in arrays that started out as `fill`: dict(n_ops, ops [n_pairs, ops_cap], ref_off, status), from
    ddh_get_cigar on every pair; plus the list of the host's raw outcomes."""
    hso = pb.a["hap_seq_off"]
    codes = capi.hpos_reference_codes(hpos)                    # the host takes MLAlignment's codes (inserted bases: -1)
    n = pb.n_pairs
    want = dict(n_ops=np.full(n, fill, np.int32), ops=np.full((n, ops_cap), fill, np.uint32), ref_off=np.full(n, fill, np.int32),
                status=np.full(n, fill, np.int32))
    outcomes = []
    for p, g, sl in pair_hpos_slices(pb):
        if pair_status is not None and pair_status[p] != 0:
            want["status"][p], want["n_ops"][p], want["ref_off"][p] = capi.DD_CIGAR_NOT_COMPUTED, 0, -1
            outcomes.append(None)
            continue
        if hap_aligned is not None and not hap_aligned[g]:
            res = -1                                           # hapRefPos.size() != hapSize: the first line of getCIGAR
        else:
            res = host_cigar(hap_ref_pos[hso[g]:hso[g + 1]], codes[sl])
        outcomes.append(res)
        if isinstance(res, int):
            want["status"][p], want["n_ops"][p], want["ref_off"][p] = HOST_CODE_TO_STATUS[res], 0, -1
            continue
        cig, ref_pos = res
        want["n_ops"][p], want["ref_off"][p] = len(cig), ref_pos
        want["status"][p] = capi.DD_CIGAR_OVERFLOW if len(cig) > ops_cap else capi.DD_CIGAR_OK
        for i, (op, ln) in enumerate(cig[:ops_cap]):
            want["ops"][p, i] = (ln << 4) | op
    return want, outcomes


def assert_equal(got, want, outcomes=None):
    """Exact equality of the four arrays; entries of `ops` a pair does not own must still hold the fill (the pairs that threw excepted:
    their count is 0 and their row is not looked at)."""
    thrown = (want["status"] >= capi.DD_CIGAR_HAP_NOT_ALIGNED) & (want["status"] <= capi.DD_CIGAR_IMPOSSIBLE)
    got = dict(got, ops=np.where(thrown[:, None], want["ops"], got["ops"]))   # a pair that threw may have written operations before it did
    for k in ("status", "n_ops", "ref_off", "ops"):
        if not np.array_equal(got[k], want[k]):
            bad = np.argwhere(got[k] != want[k])[0]
            p = int(bad[0])
            raise AssertionError("%s differs first at pair %d: got %s, want %s (status got %d want %d; host outcome %s)" % (
                k, p, got[k][p], want[k][p], got["status"][p], want["status"][p], outcomes[p] if outcomes else "?"))


def hap_ref_map(rng, hap_len, p_ins=0.01, p_del=0.01):
    """A haplotype's refHpos: reference offsets that mostly advance by one, with deletions (jumps) and insertions (-1) against the reference."""
    out, pos = [], int(rng.integers(0, 5))
    for _ in range(hap_len):
        u = rng.random()
        if u < p_ins:
            out.append(INS)
        else:
            pos += 1 if u >= p_ins + p_del else int(rng.integers(2, 7))
            out.append(pos)
    return out


def batch_hap_ref_pos(pb, seed, **kw):
    rng = np.random.default_rng(seed)
    return np.concatenate([np.asarray(hap_ref_map(rng, int(n), **kw), np.int32) for n in np.diff(pb.a["hap_seq_off"])])


def csr_batch(windows):
    """A PackedBatch with the given shape and dummy sequences: windows = [(haplotype lengths, read lengths)].  Only its index arrays matter:
    the CIGAR launch reads no base."""
    who, wro, hso, rso = [0], [0], [0], [0]
    for hl, rl in windows:
        who.append(who[-1] + len(hl)); wro.append(wro[-1] + len(rl))
        for n in hl:
            hso.append(hso[-1] + n)
        for n in rl:
            rso.append(rso[-1] + n)
    nh, nr = who[-1], wro[-1]
    return PackedBatch(win_hap_off=who, win_read_off=wro, win_hap_start=np.full(len(windows), 1000, np.uint32), hap_seq_off=hso,
                       hap_seq=np.full(hso[-1], ord("A"), np.uint8), hap_var_off=np.zeros(nh + 1, np.int32), hap_var=np.zeros(0, np.int32),
                       read_seq_off=rso, read_seq=np.full(rso[-1], ord("A"), np.uint8), read_qidx=np.zeros(rso[-1], np.uint8),
                       read_mqidx=np.zeros(nr, np.uint8), read_start=np.full(nr, 1000, np.uint32), read_flags=np.zeros(nr, np.uint8),
                       qual_table=phred_to_prob([30]), mapq_table=phred_to_prob([40]))


HAP_LEN = 400           # haplotypes of the adversarial set (hpos values stay below it)


def _hand_cases():
    """Alignments that reach the throws and the fall-through on a haplotype whose refHpos is the identity."""
    run = lambda a, n: list(range(a, a + n))
    return [
        [10],                                                   # single-base reads
        [INS], [LO], [RO],
        [LO] * 12, [INS] * 5, [DEL, LO, RO, -9],                # all-negative reads
        [LO, LO] + run(0, 20) + [RO, RO],
        run(10, 10) + [INS, INS] + run(20, 10),
        run(10, 10) + run(23, 10),
        run(10, 10) + [INS] + run(22, 8),
        run(10, 3) + [INS, 12, 13, 14],                         # INS with next - anchor = 0, then a consecutive step: "Error(3)!"
        run(10, 3) + [INS, 5, 6],                               # next - anchor < 0
        run(10, 3) + [INS, 12, INS, 13],                        # ... then reference -> insertion with op == I: "Error(2)!"
        run(10, 3) + [INS, 11, 20],                             # ... then a deletion step with op == I: "Error(4)!"
        run(10, 3) + [INS, 12, 12, 12],                         # ... then nothing but fall-throughs: ends with the insertion open
        run(10, 3) + [LO, INS, 14],                             # LO in the interior in front of an insertion: "How is this possible? (1)"
        run(10, 3) + [RO, LO, DEL] + run(13, 3),                # LO / RO / DEL in the interior: fall-throughs
        run(10, 3) + [12, 11, 10, 10] + run(11, 3),             # next - here <= 0
        [INS, INS] + run(5, 4) + [INS, INS],                    # leading / trailing insertions are clipped
    ]


def adversarial_reads(seed=11, n_random=700):
    """[hpos list]: hand cases, each also moved so that its event falls on read bases 63 / 64 / 65 and 127 / 128, and random code
    sequences of 1..200 bases."""
    rng = np.random.default_rng(seed)
    reads = []
    for c in _hand_cases():
        reads.append(c)
        pos = [v for v in c if v >= 0]
        if pos and c[0] >= 0:
            for lead in (60, 61, 62, 63, 64, 65, 124, 125, 126, 127, 128):       # a consecutive run in front: same walk, later chunk
                shift = lead + 1
                reads.append(list(range(c[0] + 1, c[0] + 1 + lead)) + [v + shift if v >= 0 else v for v in c])
    for _ in range(n_random):
        L = int(rng.choice([1, 2, 3, 17, 63, 64, 65, 66, 100, 129, 200])) if rng.random() < 0.5 else int(rng.integers(1, 201))
        h = int(rng.integers(0, HAP_LEN // 2))
        seq = []
        p_bad = float(rng.choice([0.0, 0.02, 0.1, 0.5]))
        for _i in range(L):
            u = rng.random()
            if u < p_bad:
                seq.append(int(rng.choice([INS, INS, INS, LO, RO, DEL, -7])))
            else:
                seq.append(min(max(h, 0), HAP_LEN - 1))
            h += 1 if rng.random() < 0.9 else int(rng.integers(-2, 6))
        reads.append(seq)
    return reads


def adversarial_batch(seed=11):
    """-> (pb, hpos, hap_ref_pos): two haplotypes per window (identity map; a map with indels), 16 reads per window, every pair its own
    alignment.  Inserted bases are written half as the bare -1 and half in the kernels' keyed form (DD_HPOS_INS_KEY0 - pos)."""
    rng = np.random.default_rng(seed + 1)
    reads = adversarial_reads(seed)
    per = 16
    groups = [reads[i:i + per] for i in range(0, len(reads), per)]
    pb = csr_batch([([HAP_LEN, HAP_LEN], [len(r) for r in g]) for g in groups])
    ident = np.arange(HAP_LEN, dtype=np.int32)
    other = np.asarray(hap_ref_map(np.random.default_rng(seed + 2), HAP_LEN, 0.04, 0.04), np.int32)
    hap_ref_pos = np.concatenate([ident, other] * len(groups))
    hpos = np.zeros(pb.hpos_len, np.int16)
    flat = [r for g in groups for r in g]
    nread_before = np.cumsum([0] + [len(g) for g in groups])
    for p, g, sl in pair_hpos_slices(pb):
        w = int(np.searchsorted(pb.win_pair_off, p, side="right") - 1)
        r = (p - int(pb.win_pair_off[w])) % len(groups[w])
        v = np.asarray(flat[int(nread_before[w]) + r], np.int16).copy()
        keyed = (v == INS) & (rng.random(len(v)) < 0.5)
        v[keyed] = capi.DD_HPOS_INS_KEY0 - rng.integers(1, 300, int(keyed.sum()))
        hpos[sl] = v
    return pb, hpos, hap_ref_pos


def coverage(pb, hpos, hap_ref_pos):
    """Branches of the walk the set reaches (union over pairs), checking the Python walk against ddh_get_cigar on the way."""
    hso = pb.a["hap_seq_off"]
    codes = capi.hpos_reference_codes(hpos)
    took = set()
    for p, g, sl in pair_hpos_slices(pb):
        hr = hap_ref_pos[hso[g]:hso[g + 1]]
        res, t = walk([int(x) for x in hr], [int(x) for x in codes[sl]])
        assert res == host_cigar(hr, codes[sl]), (p, res)
        took |= t
    return took
