"""Batches of the wide-deletion tests (DD_OPT_WIDE_DELETIONS: maxLengthDel above 31), and what the oracle's hpos says about them (helper; no
tests in here).

A case is about a deletion longer than the 32 states the main kernels' back-pointers hold.  Whether such a deletion is on a MAP path at
all depends on the parameters: at the default pFirstgLO = 0.01 a 100-bp read with a 40-bp deletion is placed off the haplotype instead
(all-LO costs about -9.8, the jump about -30).  So every case reads the deletion back from the ORACLE's hpos (deletions_of) before a
kernel's output is compared: a test that passed on a path without the deletion would pass on a kernel that never stores a wide choice.

Reads are two flanks of the haplotype around the deleted stretch, Q30, mapping quality 1 - 1e-4; CLI defaults otherwise.
"""
import functools

import numpy as np

from dindel_tgi_amd import capi
from dindel_tgi_amd.batch import ReadRec, Window, pack

S = 1000                      # hapStart of every window
Q30, MQ = 0.999, 0.9999


def rnd(rng, n):
    return "".join(rng.choice(list("ACGT"), n))


def params(mld, pFirstgLO=0.999, **kw):
    p = capi.params_cli_defaults()
    p.maxLengthDel = mld
    p.pFirstgLO = pFirstgLO
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def del_read(hap, at, n_del, L, left=None):
    """A read of L bases: `left` bases (default L / 2) ending at haplotype base `at` (0-based, exclusive), then the bases behind the
    deleted stretch hap[at:at + n_del]."""
    left = L // 2 if left is None else left
    seq = hap[at - left:at] + hap[at + n_del:at + n_del + (L - left)]
    assert len(seq) == L, (len(seq), L)
    return ReadRec(seq, [Q30] * L, MQ, S + at - left)


def plain_read(hap, off, L):
    return ReadRec(hap[off:off + L], [Q30] * L, MQ, S + off)


def deletions_of(hpos_row):
    """[(first deleted haplotype base, 0-based; length)] of one pair's hpos (the library's codes: negative = off the haplotype or inserted)."""
    out = []
    on = [(b, int(h)) for b, h in enumerate(hpos_row) if h >= 0]
    for (b0, h0), (b1, h1) in zip(on, on[1:]):
        if b1 == b0 + 1 and h1 - h0 > 1:
            out.append((h0 + 1, h1 - h0 - 1))
    return out


def pair_hpos(pb, arrs, w, h, r):
    """hpos of window w's haplotype h (index within the window) and read r (index within the window)."""
    ro = pb.a["win_read_off"]
    so = pb.a["read_seq_off"]
    r0, r1 = int(ro[w]), int(ro[w + 1])
    SL = int(so[r1]) - int(so[r0])
    base = int(pb.win_hpos_off[w]) + h * SL + (int(so[r0 + r]) - int(so[r0]))
    return arrs["hpos"][base:base + int(so[r0 + r + 1]) - int(so[r0 + r])]


def longest_deletion(pb, arrs, w, h, r):
    d = deletions_of(pair_hpos(pb, arrs, w, h, r))
    return max((n for _at, n in d), default=0)


# ---- (a) boundaries of the field: Hs 200, three haplotypes, 12 reads of 100 bp, 4 of them with a 40-bp deletion --------------------
A_MLDS = (32, 39, 40, 45, 63, 64, 65, 200, 201)


@functools.lru_cache(maxsize=None)
def case_a():
    rng = np.random.default_rng(4001)
    hap = rnd(rng, 200)
    haps = [hap, hap[:120] + hap[123:], hap[:30] + hap[31:]]          # 200, 197 and 199 bp: at maxLengthDel 201 every pair is "hapSize error."
    # the deletions start at 50, 60, 70, 80: each read spans 100 + 40 haplotype bases
    reads = [del_read(hap, 50 + 10 * i, 40, 100) for i in range(4)] + [plain_read(hap, 12 * i, 100) for i in range(8)]
    return pack([Window(S, haps, reads)])


# ---- (b) crossing 6 bits and 8 bits ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_b70():
    rng = np.random.default_rng(4002)
    hap = rnd(rng, 300)
    return pack([Window(S, [hap, hap[:200] + hap[202:]], [del_read(hap, 100, 70, 160), plain_read(hap, 40, 160), del_read(hap, 120, 70, 160)])])


@functools.lru_cache(maxsize=None)
def case_b260():
    """One window x 2 haplotypes x 3 reads, 900-bp haplotypes (K = 4), 560-bp reads: the largest single pair of the suite."""
    rng = np.random.default_rng(4003)
    hap = rnd(rng, 900)
    return pack([Window(S, [hap, hap[:700] + "A" + hap[700:]], [del_read(hap, 300, 260, 560), plain_read(hap, 100, 560), del_read(hap, 290, 260, 560)])])


# ---- (c) K builds and clipping --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_c(hs):
    """Haplotypes of hs bp (254: numS = 256, K = 1; 255: K = 2), pFirstgLO = 0.5.  A read whose alignment starts at haplotype base 1 and
    one whose alignment ends at the last base, each with a 40-bp deletion behind / in front of a flank of C_FLANK bases (a flank shorter
    than the deletion is cheaper as an insertion: -0.5 per inserted base against -0.5 per deleted one, so no deletion with a one-base
    flank is ever on a MAP path); the same two with 20 more bases overhanging the haplotype's end; a 50-bp deletion in the middle."""
    rng = np.random.default_rng(4100 + hs)
    hap = rnd(rng, hs)
    F = C_FLANK
    left = hap[:F] + hap[F + 40:2 * F + 40]                       # deletion (F, 40), alignment from base 1
    right = hap[hs - 2 * F - 40:hs - F - 40] + hap[hs - F:]       # deletion (hs - F - 40, 40), alignment up to the last base
    reads = [ReadRec(left, [Q30] * len(left), MQ, S), ReadRec(right, [Q30] * len(right), MQ, S + hs - 2 * F - 40),
             ReadRec(rnd(rng, 20) + left, [Q30] * (len(left) + 20), MQ, S - 20),
             ReadRec(right + rnd(rng, 20), [Q30] * (len(right) + 20), MQ, S + hs - 2 * F - 40),
             del_read(hap, 100, 50, 120), plain_read(hap, 60, 100)]
    return pack([Window(S, [hap, hap[:150] + hap[152:]], reads)])


C_FLANK = 55


@functools.lru_cache(maxsize=None)
def case_c40():
    """maxLengthDel = Hs on a 40-bp haplotype: every candidate loop is clipped at every position."""
    rng = np.random.default_rng(4140)
    hap = rnd(rng, 40)
    reads = [ReadRec(hap[:4] + hap[36:], [Q30] * 8, MQ, S), plain_read(hap, 3, 30), ReadRec(hap[:15] + hap[25:], [Q30] * 30, MQ, S),
             ReadRec(rnd(rng, 10) + hap[:12] + hap[30:] + rnd(rng, 8), [Q30] * 40, MQ, S - 10)]
    return pack([Window(S, [hap, hap[:20] + hap[21:]], reads)])


# ---- (d) ties over many equal candidates ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_d():
    """(ACGT) x 60 between two 60-bp flanks (longer than the deletions, or the flank is cheaper as an insertion); reads missing 32, 36 and 48
    bases of the repeat: every placement of the deletion within the repeat scores alike."""
    hap = "ACGT" * 60
    rng = np.random.default_rng(4200)
    flankL, flankR = rnd(rng, 60), rnd(rng, 60)
    full = flankL + hap + flankR
    reads = []
    for n_del in D_DELS:
        short = flankL + "ACGT" * ((240 - n_del) // 4) + flankR
        reads += [ReadRec(short, [Q30] * len(short), MQ, S), ReadRec(short[20:-10], [Q30] * (len(short) - 30), MQ, S + 20)]
    return pack([Window(S, [full, full[:100] + full[104:]], reads)])


D_DELS = (32, 36, 48)


# ---- (e) later items of a workgroup, and placeholders ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_e():
    """4 windows x 4 haplotypes x 40 reads of 36 bp on 120-bp haplotypes (640 pairs: more than the 512 workgroups of the grid), then an
    empty-read window and an over-limit window, and a window of reads without a haplotype."""
    rng = np.random.default_rng(4300)
    ws = []
    for _w in range(4):
        hap = rnd(rng, 120)
        haps = [hap, hap[:60] + hap[62:], hap[:40] + "C" + hap[40:], hap[:20] + hap[60:]]
        reads = [plain_read(hap, int(rng.integers(0, 84)), 36) for _ in range(34)] + \
                [ReadRec(hap[2 + i:20 + i] + hap[60 + i:78 + i], [Q30] * 36, MQ, S + 2 + i) for i in range(6)]
        ws.append(Window(S, haps, reads))
    h2 = rnd(rng, 100)
    ws.append(Window(S, [h2, h2[:50] + h2[51:]], [ReadRec("", [], MQ, S), plain_read(h2, 10, 36)]))
    ws.append(Window(S, [rnd(rng, 5000)], [plain_read(h2, 0, 50), plain_read(h2, 20, 50)]))
    ws.append(Window(S, [], [plain_read(h2, 0, 40)]))
    return pack(ws)


# ---- (f) the --faster entries -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_f():
    rng = np.random.default_rng(4400)
    hap = rnd(rng, 150)
    reads = [plain_read(hap, int(rng.integers(0, 50)), 100) for _ in range(10)] + [del_read(hap, 60, 5, 80)]
    return pack([Window(S, [hap, hap[:70] + hap[73:], hap[:30]], reads)])


@functools.lru_cache(maxsize=None)
def oracle(name, mld, pFirstgLO=0.999, faster=False, arg=None):
    """The oracle's arrays of a case (read-only; one run, shared)."""
    from tests import _oracle
    pb = globals()[name](arg) if arg is not None else globals()[name]()
    want = _oracle.batch(params(mld, pFirstgLO), pb, nthreads=16, faster=faster)
    for a in want.values():
        a.setflags(write=False)
    return want
