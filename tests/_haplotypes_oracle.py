"""A literal restatement of the reference's empirical haplotype distribution and of the iterator that makes candidate haplotypes from it.

HaplotypeDistribution (constructor, insertRead, insertSeq's four cases with their recursion, splitBlock, newBlock's sort, deleteBlock,
setFrequencies), HapBlock (the splitting constructor, insert) and HDIterator2 (setupBlocks, setThresholds, the odometer,
generateHapsWithAlignedVariants) are restated statement by statement, one segment at a time, so that the product's closed form
(host/haplotypes.cpp, csrc/hapdist_kernel.hip) has something sequential to be compared against.  It is a restatement, not the reference:
the reference's own code needs Boost and bam.h and cannot be built here, so parity with it is unpinned.

A window: rs, ref (bytes of [rs, re]) and reads = [(pos, flag, [(op, len), ...], letters)] in getReads' order.
"""
import math

REF, NORMAL, IN, DEL = 1, 2, 4, 8
BLOCK_NORMAL, BLOCK_INSERT = 0, 1
M, I, D, N, S, H, P = 0, 1, 2, 3, 4, 5, 6
FMUNMAP = 8


class Thrown(Exception):
    """throw string(...) of the reference"""


class Hap:
    def __init__(self, type_=NORMAL, seq=b""):
        self.type, self.seq, self.freq = type_, bytes(seq), 0.0

    def sub(self, pos0, n):
        h = Hap(self.type, self.seq[pos0:pos0 + n])
        h.freq = self.freq
        return h


class Block:
    """HapBlock: `haps` maps the sequence to [count, Hap]; iteration order is the map's (sorted by sequence)."""

    def __init__(self):
        self.pos0 = self.pos1 = 0
        self.type = BLOCK_NORMAL
        self.haps = {}

    @classmethod
    def from_hap(cls, h, start):
        b = cls()
        b.pos0, b.pos1 = start, start + len(h.seq) - 1
        assert b.pos1 >= b.pos0
        b.haps[h.seq] = [1, Hap(h.type, h.seq)]
        return b

    @classmethod
    def from_block(cls, hb, start, length):
        assert hb.pos1 >= start + length - 1
        b = cls()
        b.pos0, b.pos1 = start, start + length - 1
        for seq in sorted(hb.haps):
            cnt, h = hb.haps[seq]
            nh = h.sub(start - hb.pos0, length)
            hit = b.haps.get(nh.seq)
            if hit is None:
                b.haps[nh.seq] = [cnt, nh]
            else:
                if nh.type == REF:
                    hit[1].type = REF
                hit[0] += cnt
        return b

    def insert(self, h):
        hit = self.haps.get(h.seq)
        if hit is None:
            self.haps[h.seq] = [1, Hap(h.type, h.seq)]
        else:
            if h.type == REF:
                hit[1].type = REF
            hit[0] += 1

    def length(self):
        return self.pos1 - self.pos0 + 1

    def set_frequencies(self):
        total = sum(c for c, _ in self.haps.values())
        for c, h in self.haps.values():
            h.freq = float(c) / float(total)

    def entries(self):
        return [(seq, self.haps[seq][0], self.haps[seq][1].type == REF) for seq in sorted(self.haps)]


def _sort_key(b):
    return (1, 0) if b is None else (0, b.pos0)


class Distribution:
    def __init__(self, ref, rs):
        self.blocks = []                  # hapBlocks: sorted by start, None at the back
        self.insertions = {}
        bs = 4
        add = 0 if len(ref) % bs == 0 else 1
        for x in range(len(ref) // bs + add):
            self.insert_seq(Hap(REF, ref[x * bs:x * bs + bs]), rs + x * bs)

    def new_block(self, hb):
        if None in self.blocks:
            self.blocks[self.blocks.index(None)] = hb
        else:
            self.blocks.append(hb)
        self.blocks.sort(key=_sort_key)

    def delete_block(self, idx):
        self.blocks[idx] = None
        if len(self.blocks) > 1 and idx != len(self.blocks) - 1:
            self.blocks[idx] = self.blocks[-1]
            self.blocks[-1] = None

    def update_block(self, hb, seq, start):
        if len(seq.seq) != hb.length() or start != hb.pos0:
            raise Thrown("updateBlock-seq mismatch.")
        hb.insert(seq)

    def split_block(self, idx, seq, start):
        if len(seq.seq) == 0:
            raise Thrown("Empty haplotype!")
        end = start + len(seq.seq) - 1
        block = self.blocks[idx]
        if start < block.pos0 or end > block.pos1:
            raise Thrown("seq outside of block boundaries")
        len_a = start - block.pos0
        len_b = len(seq.seq)
        len_c = 0 if block.pos1 == end else block.pos1 - end
        hb_a = Block.from_block(block, block.pos0, len_a) if len_a else None
        hb_b = Block.from_block(block, block.pos0 + len_a, len_b)
        hb_c = Block.from_block(block, hb_b.pos1 + 1, len_c) if len_c else None
        self.delete_block(idx)
        self.new_block(hb_b)
        self.update_block(hb_b, seq, start)
        if len_a:
            self.new_block(hb_a)
        if len_c:
            self.new_block(hb_c)

    def first_overlapping(self, start, end):
        x = 0
        while x < len(self.blocks) and self.blocks[x] is not None:
            hb = self.blocks[x]
            if hb.pos1 >= start and hb.pos0 <= end:
                return x
            x += 1
        return -1

    def insert_seq(self, seq, start):
        if seq.type in (NORMAL, REF, DEL):
            n = len(seq.seq)
            end = start + n - 1
            idx = self.first_overlapping(start, end)
            if idx != -1:
                block = self.blocks[idx]
                if block.pos0 < start:
                    if end > block.pos1:                               # type A
                        overlap = block.pos1 - start + 1
                        self.split_block(idx, seq.sub(0, overlap), start)
                        self.insert_seq(seq.sub(overlap, n), start + overlap)
                    else:                                              # type B
                        self.split_block(idx, seq, start)
                elif block.pos1 > end:                                 # type C
                    overlap = end - block.pos0 + 1
                    self.split_block(idx, seq.sub(n - overlap, overlap), block.pos0)
                    if overlap < n:
                        self.new_block(Block.from_hap(seq.sub(0, n - overlap), start))
                else:                                                  # type D
                    len_a = block.pos0 - start
                    len_b = block.pos1 - block.pos0 + 1
                    len_c = end - block.pos1
                    if len_a:
                        self.new_block(Block.from_hap(seq.sub(0, len_a), start))
                    self.update_block(block, seq.sub(len_a, len_b), start + len_a)
                    if len_c:
                        self.insert_seq(seq.sub(len_a + len_b, len_c), start + len_a + len_b)
            else:
                self.new_block(Block.from_hap(seq, start))
        elif seq.type == IN:
            hb = self.insertions.get(start)
            if hb is None:
                hb = Block.from_hap(seq, start)
                hb.type = BLOCK_INSERT
                hb.insert(Hap(REF))
                self.insertions[start] = hb
            else:
                hb.insert(seq)
        else:
            raise Thrown("Cannot handle this case.")

    def insert_read(self, read):
        pos, flag, ops, letters = read
        if flag & FMUNMAP:
            return
        l = 0
        ref_pos = pos
        lastop = -1
        last_pos = ref_pos
        for op, length in ops:
            seq = Hap(NORMAL)
            if op in (I, M, S):
                seq.seq = bytes(letters[l:l + length])
                if len(seq.seq) != length:
                    raise Thrown("CIGAR longer than the read")     # the reference reads past the record here
                l += length
            elif op == D:
                seq.seq = b"#" * length
            seq.type = IN if op == I else DEL if op == D else NORMAL
            if len(seq.seq):
                if seq.seq[0:1] == b"#":
                    if len(seq.seq) > 30:
                        length = 30
                    seq.seq = bytes([ord("#") + length])
                self.insert_seq(seq, ref_pos)
            if lastop != -1 and lastop != I:
                if last_pos == ref_pos and lastop != S and lastop != H:
                    raise Thrown("Mag niet.")
                for p in range(last_pos, ref_pos):
                    hb = self.insertions.get(p)
                    if hb is not None:
                        hb.insert(Hap(IN))
            last_pos = ref_pos
            if op in (M, D, N):
                ref_pos += length
            elif op not in (I, S, H):
                raise Thrown("I don't know how to smoke this CIGAR")
            lastop = op

    def set_frequencies(self):
        for hb in self.blocks:
            if hb is not None:
                hb.set_frequencies()
        for hb in self.insertions.values():
            hb.set_frequencies()


def distribution(rs, ref, reads):
    """The distribution getHaplotypes builds (DInDel.cpp:1534-1540); raises Thrown."""
    hd = Distribution(bytes(ref), rs)
    for rd in reads:
        hd.insert_read(rd)
    hd.set_frequencies()
    return hd


def window_table(rs, ref, reads):
    """The part of the distribution the product computes, in canonical form: ("ok", blocks, insertions, left) with
    blocks = [(start - rs, length, [(bytes, count, is_ref)])] for the blocks inside [rs, rs + len(ref)), insertions the same for the
    insertion positions inside it (sorted by position), left = bit 0: a block ends at rs - 1, bit 1: a block starts left of rs;
    or ("throw", message)."""
    try:
        hd = distribution(rs, ref, reads)
    except Thrown as e:
        return ("throw", str(e))
    re_ = rs + len(ref) - 1
    blocks = [(hb.pos0 - rs, hb.length(), hb.entries()) for hb in hd.blocks if hb is not None and hb.pos0 >= rs and hb.pos1 <= re_]
    ins = [(p - rs, hd.insertions[p].entries()) for p in sorted(hd.insertions) if rs <= p <= re_]
    left = 0
    for hb in hd.blocks:
        if hb is not None and hb.pos0 < rs:
            left |= 2
            if hb.pos1 == rs - 1:
                left |= 1
    return ("ok", blocks, ins, left)


# ---- HDIterator2 ----------------------------------------------------------------------------------------------------------------------

class _HB:
    def __init__(self):
        self.haps, self.start, self.end, self.type = [], 0, 0, BLOCK_NORMAL


class Iterator2:
    def __init__(self, hd, max_hap, pos, left, right):
        self.list = []
        self.hbs = []
        self.setup_blocks(hd, left, right)
        self.set_thresholds(max_hap)

    def setup_blocks(self, hd, left, right):
        bl = hd.blocks
        for x in range(len(bl)):
            if bl[x] is None:
                continue
            if x and bl[x - 1].pos1 > bl[x].pos0:
                raise Thrown("Blocks are overlapping.")
            if bl[x].pos0 >= left and bl[x].pos1 <= right:
                if x == 0:
                    raise Thrown("undefined: hapBlocks[-1]")          # the reference reads in front of its vector here
                if bl[x - 1].pos1 + 1 != bl[x].pos0:
                    raise Thrown("Blocks are not consecutive.")
                self.list.append(bl[x])
        lit = 0
        for p in sorted(hd.insertions):
            ins = hd.insertions[p]
            if ins.pos0 >= left:
                for lit2 in range(lit, len(self.list)):
                    if self.list[lit2].pos0 >= p:
                        self.list.insert(lit2, ins)
                        lit = lit2 + 1                                  # the iterator still points at the block behind the new one
                        break
        for hb in self.list:
            e = _HB()
            for seq in sorted(hb.haps):
                h = hb.haps[seq][1]
                c = Hap(h.type, h.seq)
                c.freq = h.freq
                e.haps.append(c)
            e.start, e.end, e.type = hb.pos0, hb.pos1, hb.type
            if e.type == BLOCK_INSERT:
                e.end = e.start - 1
            assert any(h.type == REF for h in e.haps)
            self.hbs.append(e)
        if not self.hbs:
            raise Thrown("Not enough blocks.")

    def set_thresholds(self, max_hap):
        hbs = self.hbs
        min_freq = [0.0] * len(hbs)
        elim = [1] * len(hbs)
        log_nh = 0.0
        for e in hbs:
            log_nh += math.log(float(len(e.haps)))
        log_mh = math.log(float(max_hap))
        if log_mh < 0.0:
            log_mh = 0.0
        erased = True
        while log_nh > log_mh and erased:
            erased = False
            for x, e in enumerate(hbs):
                mf = 2.0
                for h in e.haps:
                    if h.type != REF and h.freq < mf:
                        mf = h.freq
                if len(e.haps) <= 1:
                    min_freq[x] = 2.0
                    elim[x] = 0
                else:
                    min_freq[x] = mf
            y = min_freq.index(min(min_freq))
            if elim[y] == 0:
                break
            for i, h in enumerate(hbs[y].haps):
                if h.type != REF and h.freq <= min_freq[y]:
                    del hbs[y].haps[i]
                    erased = True
                    break
            log_nh = 0.0
            for e in hbs:
                log_nh += math.log(float(len(e.haps)))
        self.max = [len(e.haps) for e in hbs]
        self.log_num_hap = log_nh
        for e in hbs:
            if not any(h.type == REF for h in e.haps):
                raise Thrown("Cannot find reference sequence.")

    def start(self):
        return self.list[0].pos0

    def end(self):
        return self.list[-1].pos1

    def generate(self, variants, change_ins_to_n=False):
        """variants: [(start_hap, kind, seq, add_comb)] in the order of AlignedCandidates::variants; kind "DEL" (seq = the deleted
        bases, its length counts), "INS" (seq = the inserted bases) or "SNP" (seq = "X=>Y": seq[3] is the new base)."""
        hbs = self.hbs
        vec_hap, vec_ref_pos = [], []
        it = [0] * len(hbs)
        last = False
        while not last:
            hap = bytearray()
            ref_pos = []
            for x, e in enumerate(hbs):
                h = e.haps[it[x]]
                length = e.end - e.start + 1
                if e.type == BLOCK_NORMAL:
                    p = e.start
                    has_del = False
                    for c in h.seq:
                        if 35 <= c < 65:
                            has_del = True
                        ref_pos.append(p)
                        p += 1
                    if not has_del and len(h.seq) != length:
                        raise Thrown("What's going on here?")
                else:
                    ref_pos.extend([-1] * len(h.seq))
                hap += h.seq
            y = 0
            while y < len(hap):
                c = hap[y]
                if 35 <= c < 65:
                    n = c - ord("#")
                    if n > len(hap) - y:
                        n = len(hap) - y
                    del hap[y:y + n]
                    del ref_pos[y:y + n]
                else:
                    y += 1
            vec_hap.append(bytes(hap))
            vec_ref_pos.append(ref_pos)
            x = 0
            while x < len(it):
                it[x] += 1
                if it[x] != self.max[x]:
                    break
                it[x] = 0
                if x == len(it) - 1:
                    last = True
                x += 1
        for ac in (1, 0):
            num_hap = len(vec_hap)
            add_comb = ac == 1
            for start_hap, kind, seq, var_comb in variants:
                if add_comb:
                    num_hap = len(vec_hap)
                if bool(var_comb) != add_comb:
                    continue
                for h in range(num_hap):
                    hap = bytearray(vec_hap[h])
                    ref_pos = list(vec_ref_pos[h])
                    if start_hap not in ref_pos:
                        continue
                    idx = ref_pos.index(start_hap)
                    changed = False
                    if kind == "DEL":
                        del hap[idx:idx + len(seq)]
                        del ref_pos[idx:idx + len(seq)]
                        changed = True
                    elif kind == "INS":
                        hap[idx:idx] = b"N" * len(seq) if change_ins_to_n else bytes(seq)
                        ref_pos[idx:idx] = [-1] * len(seq)
                        changed = True
                    elif kind == "SNP":
                        if hap[idx] != seq[3]:
                            hap[idx] = seq[3]
                            changed = True
                    if changed:
                        vec_hap.append(bytes(hap))
                        vec_ref_pos.append(ref_pos)
        return sorted(set(vec_hap))


def get_haplotypes(rs, ref, reads, pos, left, right, variants, max_hap=8, skip_max_hap=200, max_hap_read_prod=10000000,
                   change_ins_to_n=False):
    """DetInDel::getHaplotypes up to alignHaplotypes (DInDel.cpp:1526-1592): ("ok", leftPos, rightPos, [haplotype bytes]),
    ("skip", message tail) for the two `too many haplotypes` returns, or ("throw", message)."""
    try:
        hd = distribution(rs, ref, reads)
        hdi = Iterator2(hd, max_hap, pos, left, right)
        if hdi.log_num_hap > math.log(skip_max_hap):
            return ("skip", "too many haplotypes [>exp(")
        haps = hdi.generate(variants, change_ins_to_n)
        if len(haps) > skip_max_hap or len(haps) * len(reads) > max_hap_read_prod:
            return ("skip", "too many haplotypes [>%d]" % len(haps))
        return ("ok", hdi.start(), hdi.end(), haps)
    except Thrown as e:
        return ("throw", str(e))
