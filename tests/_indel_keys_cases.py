"""Shared by the tests of the --faster model's indel-map key count (tests/test_indel_keys_cpu.py, tests/test_gpu_indel_keys.py): the count
restated in Python, unlike the C header (a plain loop with a set), and alignments no traceback emits."""
import numpy as np

from dindel_tgi_amd import capi
from tests import _cigar_cases as cc

INS, DEL, LO, RO = -1, -2, -3, -4
CAP, OVERFLOW, NOT_COMPUTED = capi.DD_INDEL_KEYS_CAP, capi.DD_INDEL_KEYS_OVERFLOW, capi.DD_INDEL_KEYS_NOT_COMPUTED


def keyed(pos):
    """An inserted base as the kernels write it: DD_HPOS_INS_KEY0 - pos."""
    return capi.DD_HPOS_INS_KEY0 - pos


def is_ins(v):
    return v == INS or v < capi.DD_HPOS_INS_KEY0


def count_keys(hp):
    """The size of the indel map rebuildAlignmentFaster would build from hp (any int16 content), or OVERFLOW beyond 64 keys."""
    hp = [int(v) for v in hp]
    L, keys, lhp, b = len(hp), set(), 1, 0
    while b < L:
        c = hp[b]
        if is_ins(c):
            while b < L and is_ins(hp[b]):
                b += 1
            keys.add(lhp if c == INS else capi.DD_HPOS_INS_KEY0 - c)
            continue
        if c >= 0:
            lhp = c + 1
            if b < L - 1 and hp[b + 1] >= 0 and hp[b + 1] - c > 1:
                keys.add(c + 1)
        b += 1
    return len(keys) if len(keys) <= CAP else OVERFLOW


def run(a, n):
    return list(range(a, a + n))


def _hand_cases():
    """[hpos list]: the cases the issue names."""
    c = []
    for n in (1, 2, 63, 64, 65, 128, 129, 130):                               # read lengths around the chunk ends
        c += [run(5, n), [INS] * n, [keyed(9)] * n, [LO] * n, run(5, n - 1) + [INS], [INS] + run(5, n - 1), [v * 2 for v in run(0, n)]]
    c += [run(0, 64) + run(70, 30), run(0, 128) + run(140, 2), run(0, 63) + run(70, 30), run(0, 127) + run(131, 3)]    # deletion over 63|64, 127|128, 62|63, 126|127
    for start in (62, 63, 64, 126, 127, 128):                                 # an insertion run that starts there; runs of 1, 2 and 4 bases span the chunk end or not
        for n in (1, 2, 4):
            c += [run(0, start) + [INS] * n + run(start, 20), run(0, start) + [keyed(start)] * n + run(start, 20),
                  run(0, start) + [keyed(start + 7), INS, keyed(3)][:n] + run(start, 20)]
    c += [[INS, INS] + run(3, 40) + [INS], [keyed(4)] + run(4, 10) + [keyed(14), keyed(14)]]      # a run at the read's start and at its end
    c += [run(10, 5) + [LO] * 70 + [INS, INS] + run(15, 3),                   # a bare run whose lhp comes from the chunk before ...
          run(10, 60) + [RO] * 80 + [INS] + [DEL] * 70 + [INS], [INS], [INS, 7, INS]]             # ... from two chunks before; at base 0 (lhp = 1)
    c += [[keyed(5), LO, keyed(5)], [INS, LO, INS], [keyed(5), INS, LO, INS, keyed(5), RO, keyed(5)],   # the same key twice: counted once
          [4, INS, LO, keyed(5)], [keyed(11), 10, 15], [10, 15, keyed(11)], [10, INS, 10, 15],           # a deletion key equal to an insertion key
          [50, 10, 40, 3, 3, 90, 2, 1, 0, 0, 200], [9, 8, 7, 6, 5], [5, 5, 5, 7, 7, 9],                 # non-monotone positions
          [3, LO, 9, RO, 12, DEL, 20, DEL, DEL, 30, 40, LO, INS, RO, INS, DEL, keyed(2), -5, -16, 8, -15, 60],   # other codes in between
          [-32768], [32767, INS], [0, 32767], [32767, 0, 32767], [-32768, 0, -17, 5, -17], [32766, INS, 32767, INS, 0, INS],   # int16 extremes
          [0, 32767, -32768, 32766, keyed(32752), 1, INS]]
    # exactly 64 and 65 distinct keys, by deletions, by keyed runs, by bare runs; 65 events of which two share a key
    c += [[2 * i for i in range(65)], [2 * i for i in range(66)], [2 * i for i in range(200)]]
    for n in (64, 65):
        c += [sum([[keyed(100 + i), LO] for i in range(n)], []), sum([[3 * i, INS] for i in range(n)], []),
              sum([[keyed(100 + i), 3 * i, 3 * i + 2] for i in range(n // 2)], []) + ([keyed(7)] if n == 65 else [])]
    c += [sum([[keyed(100 + (i % 64)), LO] for i in range(130)], []), sum([[keyed(100 + i), LO] for i in range(64)], []) + [keyed(100)],
          [LO] * 64 + sum([[keyed(100 + i), LO] for i in range(65)], [])]
    return c


def adversarial_reads(seed=23, n_random=500):
    rng = np.random.default_rng(seed)
    reads = [list(r) for r in _hand_cases()]
    vocab = [INS, INS, DEL, LO, RO, keyed(1), keyed(7), keyed(40), -17, -16, -15, -5, -32768, 32767, 0]
    for _ in range(n_random):
        L = int(rng.integers(1, 201))
        style = rng.random()
        if style < 0.4:                                                       # anything goes
            r = [int(rng.choice(vocab)) if rng.random() < 0.4 else int(rng.integers(0, 60)) for _ in range(L)]
        elif style < 0.7:                                                     # a walk along the haplotype with events
            r, pos = [], int(rng.integers(0, 30))
            for _ in range(L):
                u = rng.random()
                if u < 0.08:
                    r.append(INS if rng.random() < 0.5 else keyed(pos))
                elif u < 0.12:
                    r.append(int(rng.choice([LO, RO, DEL])))
                else:
                    pos += 1 if u < 0.9 else int(rng.integers(2, 6))
                    r.append(pos)
        else:                                                                 # many keys: around the cap
            r = [int(rng.integers(0, 3 * L + 2)) if rng.random() < 0.7 else keyed(int(rng.integers(1, 90))) for _ in range(L)]
        reads.append(r)
    return reads


def adversarial_batch(seed=23, per=16):
    """-> (pb, hpos): two haplotypes per window, `per` reads per window; haplotype 0's pairs carry the reads as they are, haplotype 1's the
    same reads backwards (another alignment of the same length)."""
    reads = adversarial_reads(seed)
    groups = [reads[i:i + per] for i in range(0, len(reads), per)]
    pb = cc.csr_batch([([100, 100], [len(r) for r in g]) for g in groups])
    hpos = np.zeros(pb.hpos_len, np.int16)
    flat = [r for g in groups for r in g]
    for p, _g, sl in cc.pair_hpos_slices(pb):
        w = int(np.searchsorted(pb.win_pair_off, p, side="right")) - 1
        base = int(pb.win_pair_off[w])
        R = len(groups[w])
        h, r = divmod(p - base, R)
        src = flat[int(pb.a["win_read_off"][w]) + r]
        hpos[sl] = np.asarray(src if h == 0 else src[::-1], np.int16)
    return pb, hpos


def expected(pb, hpos, status=None):
    """The Python restatement over every pair of a batch: int16 [n_pairs]."""
    out = np.zeros(pb.n_pairs, np.int16)
    for p, _g, sl in cc.pair_hpos_slices(pb):
        out[p] = NOT_COMPUTED if status is not None and status[p] != 0 else count_keys(hpos[sl])
    return out
