"""Windows for the block table of the haplotype distribution: a seeded generator and hand-derived cases, shared by the CPU and the GPU
tests.  A case is (name, rs, ref, reads) with reads = [(pos, flag, [(op, len), ...], letters)] (tests/_haplotypes_oracle.py)."""
import random
import re

OPS = "MIDNSHP=X"
LETTERS = b"ACGT"


def cigar(text):
    return [(OPS.index(o), int(n)) for n, o in re.findall(r"(\d+)([MIDNSHP=X])", text)]


def genome(n, seed):
    rng = random.Random(seed)
    return bytes(rng.choice(LETTERS) for _ in range(n))


def read_from(g, pos, ops, rng=None, err=0.0, ins=None):
    """A read whose M bases copy the genome `g` (with substitution rate `err`), its I bases `ins` (or random), its S bases random."""
    rng = rng or random.Random(pos)
    out, at = bytearray(), pos
    for op, ln in ops:
        if op == 0:
            for x in range(ln):
                c = g[at + x] if 0 <= at + x < len(g) else ord("N")
                if err and rng.random() < err:
                    c = rng.choice(b"ACGTN")
                out.append(c)
        elif op == 1:
            out += (ins if ins is not None and len(ins) == ln else bytes(rng.choice(LETTERS) for _ in range(ln)))
        elif op == 4:
            out += bytes(rng.choice(LETTERS) for _ in range(ln))
        if op in (0, 2, 3):
            at += min(ln, 30) if op == 2 else ln
    return bytes(out)


G = genome(6000, 20261019)

_SHAPES = ["{a}M", "{s}S{a}M", "{a}M{s}S", "{s}S{a}M{s}S", "{s}H{a}M{s}H", "{a}M{i}I{b}M", "{a}M{d}D{b}M", "{a}M{n}N{b}M",
           "{a}M{i}I{b}M{d}D{c}M", "{i}I{a}M", "{a}M{i}I", "{a}M{i}I{s}S", "{s}S{a}M{i}I{b}M{s}S", "{a}M{d}D{b}M{i}I{c}M", "{a}M{i}I{b}M{n}N{c}M"]


def generated(n, seed, max_reads=40, wide=False):
    """n windows; every few of them carry something the reference throws on."""
    rng = random.Random(seed)
    cases = []
    for w in range(n):
        rs = rng.randrange(200, 3000)
        L = rng.randrange(300, 700) if wide else rng.choice([rng.randrange(1, 12), rng.randrange(20, 80), rng.randrange(80, 200)])
        ref = G[rs:rs + L]
        ins_sites = [rs + rng.randrange(0, L) for _ in range(2)]
        ins_strings = [bytes(rng.choice(LETTERS) for _ in range(rng.randrange(1, 5))) for _ in range(3)]
        reads = []
        for _ in range(rng.randrange(0, max_reads + 1)):
            shape = rng.choice(_SHAPES if rng.random() < 0.6 else _SHAPES[:5])
            v = dict(a=rng.randrange(1, 60), b=rng.randrange(1, 40), c=rng.randrange(1, 30), s=rng.randrange(1, 9), i=rng.randrange(1, 5),
                     d=rng.choice([1, 1, 2, 3, 7, 29, 30, 31, 40]), n=rng.randrange(1, 50))
            ops = cigar(shape.format(**v))
            pos = rng.randrange(rs - 70, rs + L + 10)
            ins = None
            if "I" in shape and rng.random() < 0.7:           # let reads share insertion sites, with one of a few strings
                site, ins = rng.choice(ins_sites), rng.choice(ins_strings)
                before = 0
                for op, ln in ops:
                    if op == 1:
                        break
                    before += ln if op in (0, 3) else min(ln, 30) if op == 2 else 0
                pos = site - before
                ops = [(op, len(ins)) if op == 1 else (op, ln) for op, ln in ops]
            flag = rng.choice([0, 0, 0, 16, 1, 3, 8, 9, 4])
            reads.append((pos, flag, ops, read_from(G, pos, ops, rng, err=rng.choice([0.0, 0.02, 0.1]), ins=ins)))
        if rng.random() < 0.1:
            reads.append((rs + 3, 0, [], b""))                 # a read with no operations
        if rng.random() < 0.06:
            bad = rng.choice(["10M2P10M", "10M0D5M", "5M0M5M", "10M3X", "4=", "10M0N4M"])
            ops = cigar(bad)
            reads.insert(rng.randrange(0, len(reads) + 1), (rs + 1, 0, ops, read_from(G, rs + 1, ops, rng)))
        cases.append(("gen%d_%d" % (seed, w), rs, ref, reads))
    return cases


def hand():
    """Hand-derived windows; what each one is about is in its name."""
    rs, L = 1000, 24
    ref = G[rs:rs + L]

    def rd(pos, text, flag=0, ins=None, err=0.0, letters=None):
        ops = cigar(text)
        return (pos, flag, ops, letters if letters is not None else read_from(G, pos, ops, random.Random(pos * 31 + len(text)), err, ins))

    snp = bytearray(G[1000:1020])
    snp[5] = ord("A") if snp[5] != ord("A") else ord("C")
    withn = bytearray(G[1002:1016])
    withn[3] = ord("N")
    cases = [
        ("zero_reads", rs, ref, []),
        ("window_not_multiple_of_4", 1001, G[1001:1001 + 23], [rd(1001, "23M")]),
        ("on_grid", rs, ref, [rd(1000, "8M"), rd(1004, "12M"), rd(1016, "8M")]),
        ("off_grid", rs, ref, [rd(1001, "6M"), rd(1003, "9M"), rd(1010, "13M")]),
        ("past_both_ends", rs, ref, [rd(980, "70M"), rd(990, "12M"), rd(1020, "30M")]),
        ("left_gap_before_window", rs, ref, [rd(960, "20M")]),                     # a block left of rs that does not touch it
        ("left_touching", rs, ref, [rd(960, "40M")]),
        ("ref_read_and_snp", rs, ref, [rd(1000, "20M"), rd(1000, "20M", letters=bytes(snp)), rd(1000, "20M", letters=bytes(snp))]),
        ("n_in_read", rs, ref, [rd(1002, "14M", letters=bytes(withn))]),
        ("leading_clip_overlaps_its_match", rs, ref, [rd(1004, "5S12M")]),
        ("trailing_clip_runs_on", rs, ref, [rd(1002, "10M6S")]),
        ("both_clips", rs, ref, [rd(1006, "3S8M4S"), rd(1006, "8M")]),
        ("hard_clips", rs, ref, [rd(1003, "5H10M5H")]),
        ("del_1_29_30_31", 1000, G[1000:1100], [rd(1002, "6M1D8M"), rd(1003, "7M29D8M"), rd(1004, "6M30D9M"), rd(1005, "6M31D9M"), rd(1006, "5M45D5M")]),
        ("del_30_on_an_A", rs, ref, [rd(G.index(b"A", 1004) - 3, "3M30D4M")]),  # '#' + 30 is 'A': counted with the reference's A
        ("ref_skip", rs, ref, [rd(1001, "5M7N6M")]),
        # (a read's last operation never counts as crossing: the clips make the matches count)
        ("ins_first_read_creates", rs, ref, [rd(1002, "6M2I8M", ins=b"GG"), rd(1001, "15M2S"), rd(1004, "12M1S"), rd(1003, "12M")]),
        ("ins_middle_read_creates", rs, ref, [rd(1001, "15M2S"), rd(1002, "6M2I8M", ins=b"GG"), rd(1004, "12M1S"), rd(1005, "3M2I9M", ins=b"GG")]),
        ("ins_last_read_creates", rs, ref, [rd(1001, "15M2S"), rd(1004, "12M1S"), rd(1002, "6M2I8M", ins=b"GG")]),
        ("ins_carrier_goes_on_behind_its_match", rs, ref, [rd(1002, "6M2I4M2D6M", ins=b"TT"), rd(1003, "5M2I3M1D3M", ins=b"TT")]),
        ("two_insertions_at_one_position", rs, ref, [rd(1002, "6M2I8M", ins=b"GG"), rd(1003, "5M3I8M", ins=b"ACA"), rd(1000, "20M2S"),
                                                     rd(1004, "4M2I2M", ins=b"GG")]),
        ("ins_at_read_start_and_end", rs, ref, [rd(1005, "2I8M", ins=b"CC"), rd(1001, "9M3I", ins=b"TGA"), rd(1000, "12M3S")]),
        ("ins_before_clip", rs, ref, [rd(1001, "9M1I4S", ins=b"A"), rd(1003, "15M")]),
        ("mate_unmapped_is_ignored", rs, ref, [rd(1001, "10M", flag=8), rd(1002, "8M1I4M", flag=9, ins=b"T"), rd(1003, "9M")]),
        ("no_operations", rs, ref, [(1004, 0, [], b""), rd(1003, "9M")]),
        ("pad_throws", rs, ref, [rd(1001, "10M"), rd(1003, "4M2P4M")]),
        ("mag_niet", rs, ref, [rd(1001, "10M"), rd(1003, "4M0D4M")]),
        ("one_position_window", 1500, G[1500:1501], [rd(1495, "12M"), rd(1500, "1M")]),
    ]
    return cases
