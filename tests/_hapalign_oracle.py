"""Independent restatement of the haplotype-to-reference alignment and of what DetInDel::alignHaplotypes / getHaplotypes make of it.
Test infrastructure only: nothing under dindel_tgi_amd/ imports it.

  * `align`: SeqAn's Gotoh alignment (seqan/graph_align/graph_align_gotoh.h, _align_gotoh and _align_gotoh_trace) with
    Score<int>(-1, -460, -100, -960), written unlike the kernel: whole columns at a time with numpy (the vertical gap as a running maximum
    over the column), the full matrix of trace nibbles kept, the tie bits derived from the finished values.  tests/test_hapalign_cpu.py pins
    it against the library's own output on every fixture of tests/golden/hapalign_seqan.json.
  * `convert`, `flanking`, `add_ref_variant`, `window`: convertAlignment (ObservationModelSeqAn.hpp:142-269),
    Realign::getFlankingCoordinatesBetter (:37-139), Haplotype::addRefVariant (Haplotype.hpp:201-251), the rest of alignHaplotypes
    (DInDel.cpp:1488-1510) and of getHaplotypes (:1600-1626).  Those need Haplotype.hpp (Boost) on the reference side, so this part is a
    restatement checked against the C++ restatement, not against reference output.
"""
import numpy as np

MATCH, MISMATCH, GAP_EXTEND, GAP_OPEN = -1, -460, -100, -960
INS, DEL, LO, RO = -1, -2, -3, -4          # MLAlignment.hpp:31-34
DIAG, HOR, VERT = 0, 1, 2

_CODE = np.zeros(256, np.int64)
for _c, _v in (("C", 1), ("G", 2), ("T", 3), ("U", 3)):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _v


def codes(seq):
    return _CODE[np.frombuffer(bytes(seq), np.uint8)]


def dna(seq):
    return "".join("ACGT"[c] for c in codes(seq))


def _dp(ref, hap):
    """score, initial direction and the (len1, len2) matrix of trace nibbles: tv | hor-open << 2 | vert-open << 3."""
    r, h = codes(ref), codes(hap)
    n1, n2 = len(r), len(h)
    rows = np.arange(n2 + 1, dtype=np.int64)
    M = np.where(rows == 0, 0, GAP_OPEN + GAP_EXTEND * (rows - 1))           # column 0
    H = M + GAP_OPEN - GAP_EXTEND
    trace = np.zeros((n1, n2), np.uint8)
    V = None
    for col in range(1, n1 + 1):
        top = GAP_OPEN + GAP_EXTEND * (col - 1)
        h_open, h_ext = M[1:] + GAP_OPEN, H[1:] + GAP_EXTEND
        Hn = np.maximum(h_open, h_ext)
        D = M[:-1] + np.where(h == r[col - 1], MATCH, MISMATCH)
        # vertical: V[row] = max over k < row of M[k] - 960 - 100 (row - 1 - k); a cell reached through a vertical gap never opens the best
        # one below it (960 + 960 - 100 > 960), so M[k] may be replaced by max(D[k], H[k]) and the column needs no loop
        X = np.concatenate([[top], np.maximum(D, Hn)])
        run = np.maximum.accumulate(X[:-1] - GAP_EXTEND * rows[:-1])
        V = run + GAP_OPEN + GAP_EXTEND * (rows[1:] - 1)
        Mn = np.concatenate([[top], np.maximum(X[1:], V)])
        tv = np.where(V > D, VERT, DIAG)
        tv = np.where(Hn > np.maximum(D, V), HOR, tv)
        v_prev = np.concatenate([[top + GAP_OPEN - GAP_EXTEND], V[:-1]])     # the running vert in front of each row
        v_open = Mn[:-1] + GAP_OPEN > v_prev + GAP_EXTEND
        trace[col - 1] = tv | ((h_open > h_ext).astype(np.uint8) << 2) | (v_open.astype(np.uint8) << 3)
        Hfull = np.concatenate([[0], Hn])
        M, H = Mn, Hfull
    direction = DIAG
    if H[n2] == M[n2]:
        direction = HOR
    elif V[n2 - 1] == M[n2]:
        direction = VERT
    return int(M[n2]), direction, trace


def _traceback(trace, n1, n2, direction):
    """The (tv, length) segments, last first, as _align_gotoh_trace prints them."""
    segs = []
    l1, l2 = n1, n2
    ntv = int(trace[l1 - 1, l2 - 1])
    tv = DIAG
    if direction == DIAG:
        tv = ntv & 3
    elif direction == HOR:
        if (ntv >> 2) & 1:
            l1 -= 1; segs.append((HOR, 1))
        else:
            tv = HOR
    else:
        if (ntv >> 3) & 1:
            l2 -= 1; segs.append((VERT, 1))
        else:
            tv = VERT
    seg, old = 0, tv
    while True:
        assert l1 > 0 and l2 > 0, "the source would read the trace at index -1 here"
        ntv = int(trace[l1 - 1, l2 - 1])
        if tv == DIAG:
            tv = ntv & 3
        elif tv == HOR:
            tv = DIAG if (ntv >> 2) & 1 else HOR
        else:
            tv = DIAG if (ntv >> 3) & 1 else VERT
        if tv == DIAG:
            if tv != old:
                if old == VERT:
                    l2 -= 1
                else:
                    l1 -= 1
                seg += 1
                segs.append((old, seg))
                old, seg = tv, 0
            else:
                seg += 1; l1 -= 1; l2 -= 1
        elif tv == HOR:
            if tv != old:
                segs.append((old, seg))
                if (ntv >> 2) & 1:
                    l1 -= 1; segs.append((HOR, 1)); tv = DIAG; seg = 0
                else:
                    old, seg = tv, 1; l1 -= 1
            else:
                seg += 1; l1 -= 1
        else:
            if tv != old:
                segs.append((old, seg))
                if (ntv >> 3) & 1:
                    l2 -= 1; segs.append((VERT, 1)); tv = DIAG; seg = 0
                else:
                    old, seg = tv, 1; l2 -= 1
            else:
                seg += 1; l2 -= 1
        if l1 == 0 or l2 == 0:
            break
    if seg:
        segs.append((old, seg))
    if l1:
        segs.append((HOR, l1))
    elif l2:
        segs.append((VERT, l2))
    return segs


def align(ref, hap):
    """(score, row0, row1, ref_pos): the gapped rows as text and, per haplotype base, the reference offset it is paired with, or
    -1 - (reference bases left of its column) when it faces a gap."""
    ref, hap = bytes(ref), bytes(hap)
    score, direction, trace = _dp(ref, hap)
    segs = _traceback(trace, len(ref), len(hap), direction)
    r, h = dna(ref), dna(hap)
    row0, row1, pos = [], [], []
    i = j = 0
    for tv, n in reversed(segs):                     # _pump_trace_2_Align reads the trace backwards
        if tv == DIAG:
            row0.append(r[i:i + n]); row1.append(h[j:j + n]); pos.extend(range(i, i + n)); i += n; j += n
        elif tv == HOR:
            row0.append(r[i:i + n]); row1.append("-" * n); i += n
        else:
            row0.append("-" * n); row1.append(h[j:j + n]); pos.extend([-1 - i] * n); j += n
    assert i == len(ref) and j == len(hap), (i, j)
    return score, "".join(row0), "".join(row1), np.array(pos, np.int16)


def rows_from_ref_pos(ref, hap, ref_pos):
    """Gapped rows of an alignment given as per-base reference offsets; a gap-facing base carries -1 - (reference bases left of it)."""
    r, h = dna(ref), dna(hap)
    row0, row1, nxt = [], [], 0
    for b, p in enumerate(int(v) for v in ref_pos):
        upto = p if p >= 0 else -1 - p
        row0.append(r[nxt:upto]); row1.append("-" * (upto - nxt)); nxt = upto
        if p < 0:
            row0.append("-"); row1.append(h[b])
        else:
            row0.append(r[p]); row1.append(h[b]); nxt = p + 1
    row0.append(r[nxt:]); row1.append("-" * (len(r) - nxt))
    return "".join(row0), "".join(row1)


# ---- convertAlignment and what follows it ----------------------------------------------------------------------------------------------

class Variant:
    """AlignedVariant: the string, eight coordinates and the type its string implies (Variant.hpp:43-74)."""

    def __init__(self, s, start_hap, end_hap, start_read, end_read):
        self.str = s
        self.coords = [start_hap, end_hap, start_read, end_read, start_hap, end_hap, start_read, end_read]
        if len(s) > 1 and s[0] == "-":
            self.type, self.size, self.seq = "DEL", len(s) - 1, s[1:]
        elif len(s) > 1 and s[0] == "+":
            self.type, self.size, self.seq = "INS", len(s) - 1, s[1:]
        elif len(s) == 4 and s[1:3] == "=>":
            self.type, self.size, self.seq = "SNP", 1, s
        elif s == "*REF":
            self.type, self.size, self.seq = "REF", 1, s
        else:
            raise ValueError("Unrecognized variant")

    def record(self, kind, key):
        return "V %s %d %s %s" % (kind, key, self.str, " ".join(str(c) for c in self.coords))


def flanking(ref_seq, read_len, av):
    """Realign::getFlankingCoordinatesBetter (ObservationModelSeqAn.hpp:39-138); `hap` there is the reference sequence, `read` the
    candidate haplotype.  Quirks kept: the leftward loops stop at x > 0, and an overrun of rightFlankRead assigns leftFlankRead."""
    hs = ref_seq
    start_hap, start_read = av.coords[0], av.coords[2]
    if av.type == "DEL":
        l, sh = av.size, start_hap
        orig = hs[:sh] + hs[sh + l:]
        lfh, rfh = sh - 1, sh + l
        for x in range(sh - 1, 0, -1):
            if hs[:x] + hs[x + l:] == orig:
                lfh = x - 1
        if lfh <= 0:
            lfh = 0
        for x in range(sh + 1, len(hs) - l):
            if hs[:x] + hs[x + l:] == orig:
                rfh = x + l
        lfr = start_read - (sh - lfh) + 1
        if lfr < 0:
            lfr = 0
        rfr = start_read + 1 + (rfh - sh - l)
        if rfr >= read_len:
            lfr = read_len - 1
    elif av.type == "INS":
        l, sh = av.size, start_hap
        orig = hs[:sh] + av.seq + hs[sh:]
        lfh, rfh = sh - 1, sh
        for x in range(sh - 1, 0, -1):
            if hs[:x] + orig[x:x + l] + hs[x:] == orig:
                lfh = x - 1
        if lfh <= 0:
            lfh = 0
        for x in range(sh + 1, len(hs) - l):
            if hs[:x] + orig[x:x + l] + hs[x:] == orig:
                rfh = x
        lfr = start_read - (sh - lfh) + 1
        if lfr < 0:
            lfr = 0
        rfr = start_read + l + (rfh - sh)
        if rfr >= read_len:
            lfr = read_len - 1
    else:
        lfr = max(start_read - 1, 0)
        rfr = start_read + 1
        if rfr >= read_len:
            lfr = read_len - 1
        lfh = max(start_hap - 1, 0)
        rfh = start_hap + 1
        if rfh >= len(hs):
            lfh = len(hs) - 1
    av.coords[4:8] = [lfh, rfh, lfr, rfr]


class Converted:
    pass


def convert(ref_seq, hap_seq, row0, row1):
    """convertAlignment (ObservationModelSeqAn.hpp:142-269) on the gapped rows.  ref_seq: the window's reference as text (hlen bases),
    hap_seq: the candidate haplotype (rlen bases)."""
    hlen, rlen, end = len(ref_seq), len(hap_seq), len(row0)
    ml = Converted()
    ml.align = ["R"] * hlen
    ml.hpos = [LO] * rlen
    ml.indels, ml.snps = {}, {}
    ml.relPos, ml.firstBase, ml.lastBase = 0, -1, -1
    fbfound = False
    b = rb = 0
    while b < end and row0[b] == "-":
        ml.relPos -= 1
        if row1[b] != "-":
            ml.hpos[rb] = LO
            rb += 1
        b += 1
    hb = 0
    while b < end and rb < rlen:
        if row0[b] == "-":
            if hb < hlen:
                seq = "+"
                while b < end and row0[b] == "-":
                    seq += row1[b]
                    ml.hpos[rb] = INS
                    b += 1; rb += 1
                av = Variant(seq, hb, hb, rb - len(seq) + 1, rb - 1)
                flanking(ref_seq, rlen, av)
                ml.indels[hb] = av
            else:
                ml.hpos[rb] = RO
                rb += 1; b += 1
        elif row1[b] != "-":
            if not fbfound:
                fbfound = True
                ml.firstBase = hb
            if row1[b] != row0[b]:
                av = Variant(row0[b] + "=>" + row1[b], hb, hb, rb, rb)
                flanking(ref_seq, rlen, av)
                ml.snps[hb] = av
                ml.align[hb] = row1[b]
            ml.hpos[rb] = hb
            rb += 1; b += 1; hb += 1
        else:
            seq, n = "-", 0
            while b < end and row1[b] == "-":
                seq += row0[b]
                ml.align[hb] = "D"
                b += 1; hb += 1; n += 1
            if fbfound:
                av = Variant(seq, hb - n, hb - 1, rb - 1, rb)
                flanking(ref_seq, rlen, av)
                ml.indels[hb - n] = av
    ml.lastBase = hb
    ml.align = "".join(ml.align)
    return ml


def add_ref_variant(ml, rp):
    """Haplotype::addRefVariant (Haplotype.hpp:201-251)."""
    offset = 0
    for key in sorted(ml.indels):
        if key > rp:
            break
        v = ml.indels[key]
        if v.type == "DEL":
            if key + v.size <= rp:
                offset -= v.size
            else:
                break
        if v.type == "INS":
            offset += v.size
    a = ml.align[rp]
    gt = "*REF" if a == "R" else "R=>" + a
    for m in (ml.indels, ml.snps):
        if rp not in m:
            m[rp] = Variant(gt, rp, rp, rp + offset, rp + offset)


def window(ref_seq, haps):
    """alignHaplotypes + the end of getHaplotypes for one window: the kept haplotypes as (sequence, Converted), in order; Converted.index
    is the haplotype's place in `haps`.  ref_seq, haps: text (latin-1 of the bytes)."""
    done, positions = [], set()
    for index, h in enumerate(haps):
        _, row0, row1, _ = align(ref_seq.encode("latin-1"), h.encode("latin-1"))
        ml = convert(ref_seq, h, row0, row1)
        ml.index = index
        positions.update(ml.indels)
        positions.update(ml.snps)
        start_end = ml.hpos[0] == LO or (len(ml.hpos) > 1 and ml.hpos[-1] == RO)      # DInDel.cpp:1488-1491
        if not start_end:
            done.append((h, ml))
    for rp in sorted(positions):
        for _, ml in done:
            add_ref_variant(ml, rp)
    kept, found_ref = [], False
    for h, ml in done:                                                                  # DInDel.cpp:1600-1616
        n_indels = sum(1 for v in ml.indels.values() if v.type in ("INS", "DEL"))
        n_snps = sum(1 for v in ml.snps.values() if v.type == "SNP")
        if n_indels == 0 and n_snps == 0:
            if found_ref:
                continue
            found_ref = True
        kept.append((h, ml))
    return kept


def window_records(index, left, right, kept):
    """The W / H / A / V lines of one window, as the dump of INTEGRATION section 8 writes them."""
    lines = ["W %d %d %d" % (index, left, right)]
    for h, ml in kept:
        lines.append("H " + h)
        lines.append("A" + "".join(" %d" % p for p in ml.hpos))
        for kind, m in (("I", ml.indels), ("S", ml.snps)):
            for key in sorted(m):
                lines.append(m[key].record(kind, key))
    return lines
