"""TEST INFRASTRUCTURE ONLY: the sample shared by tests/test_discover_cpu.py and tests/test_discover_driver_gpu.py, and the call of the
discovery stage inside the host library.  Two targets of 2,000 bp; 50-bp reads at about 20x as mate pairs in two read groups (two
libraries); indels implanted through the reads' CIGARs:
  chrA  a 1-bp deletion inside an 8-base homopolymer (600 ... 607), written at a different base of the run by every read that carries it,
        so that only the realignment brings them to one candidate; a 3-bp insertion at 900; a deletion at 1200 and an insertion at 1215
        (15 apart: one window at the default --minDist 20); deletions at 1500 and 1521 (21 apart: two windows, one at --minDist 25)
  chrB  a 2-bp deletion at 30 (the window's left edge is clamped to 0); a 4-bp deletion at 1400; an insertion at 1000 carried by a
        single read (gone with --minCount 2).
sample(length=6000, shift=3000) is the same sample on longer targets with every indel but the one at 30 moved 3,000 bases on: read selection
reaches back leftPos - maxInsertSize - 200 in unsigned arithmetic (DInDel.cpp:928), so without a library file (maxInsertSize 2,000) every
window of a 2,000-base target wraps around and is skipped for want of reads; the longer targets' windows are called."""
import ctypes as C
import os
import random

from dindel_tgi_amd import hostlib
from tests import _bamwriter, _candidates_cases as cases
from tests.test_glf_vcf_cpu import write_fasta

READ = 50
RUN = (600, 608)                                      # the homopolymer of chrA

# (position, kind, payload: deleted length or inserted letters, fraction of the fragments that carry it)
def events(shift=0):
    return {"chrA": [("run", "del", 1, 0.5), (900 + shift, "ins", "GAT", 1.0), (1200 + shift, "del", 2, 0.5), (1215 + shift, "ins", "C", 0.5),
                     (1500 + shift, "del", 1, 0.5), (1521 + shift, "del", 3, 0.5)],
            "chrB": [(30, "del", 2, 0.6), (1400 + shift, "del", 4, 0.5)]}


def _target(rng, n, run=None):
    s = [rng.choice("ACGT") for _ in range(n)]
    for i in range(3, n):                             # no homopolymer longer than 3 but the planted one
        if s[i] == s[i - 1] == s[i - 2] == s[i - 3]:
            s[i] = "ACGT"[("ACGT".index(s[i]) + 1 + i % 3) % 4]
    if run:
        s[run[0] - 1], s[run[1]] = "C", "G"
        s[run[0]:run[1]] = "A" * (run[1] - run[0])
    return "".join(s)


def _read(ref, pos, events):
    """(sequence, CIGAR) of a READ-base read whose alignment starts at `pos` and carries `events` ({position: (kind, payload)}); an
    event closer than 6 read bases to either end of the read is left out"""
    seq, ops, r, done = [], [], pos, set()

    def op(c, n):
        if ops and ops[-1][0] == c:
            ops[-1][1] += n
        else:
            ops.append([c, n])
    while len(seq) < READ:
        ev = events.get(r)
        if ev and r not in done:
            done.add(r)
            kind, payload = ev
            room = READ - len(seq) - (len(payload) if kind == "ins" else 0)
            if len(seq) >= 6 and room >= 6:
                if kind == "del":
                    op("D", payload)
                    r += payload
                else:
                    seq.extend(payload)
                    op("I", len(payload))
                continue
        seq.append(ref[r])
        op("M", 1)
        r += 1
    return "".join(seq), "".join("%d%s" % (n, c) for c, n in ops)


def sample(tmp, seed=1810, depth=20, length=2000, shift=0):
    """dict(bam, bams (the same reads dealt out over two files), list (their --bamFiles file), fasta, targets, names, shift)"""
    rng = random.Random(seed)
    names = ["chrA", "chrB"]
    run = (RUN[0] + shift, RUN[1] + shift)
    EVENTS = events(shift)
    targets = {"chrA": _target(rng, length, run), "chrB": _target(rng, length)}
    for name in names:                                # every planted indel is its own canonical (leftmost) form: the base in front differs
        s = list(targets[name])
        for at, kind, payload, _ in EVENTS[name] + ([(1000 + shift, "ins", "TT", 0)] if name == "chrB" else []):
            if at != "run":
                last = s[at + payload - 1] if kind == "del" else payload[-1]
                if s[at - 1] == last:
                    s[at - 1] = "ACGT"[("ACGT".index(last) + 1) % 4]
        targets[name] = "".join(s)
    fasta = os.path.join(str(tmp), "discover.fa")
    write_fasta(fasta, [(n, targets[n]) for n in names])
    header = "@HD\tVN:1.0\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, length) for n in names) + "@RG\tID:g1\tLB:libOne\tSM:s\n@RG\tID:g2\tLB:libTwo\tSM:s\n"
    records = []
    for tid, name in enumerate(names):
        ref = targets[name]
        for f in range(length * depth // (2 * READ)):
            isize = max(2 * READ + 10, int(rng.gauss(250, 15)))
            p1 = rng.randrange(0, length - isize - 12)
            p2 = p1 + isize - READ
            carried = {}
            for at, kind, payload, frac in EVENTS[name]:
                if rng.random() < frac:
                    carried[rng.randrange(*run) if at == "run" else at] = (kind, payload)
            for k, (p, flag) in enumerate(((p1, 99), (p2, 147))):
                seq, cigar = _read(ref, p, carried)
                records.append((tid, dict(qname="f%d_%d" % (tid, f), flag=flag, pos=p, mapq=60, cigar=cigar, seq=seq, qual=[30] * READ, mtid=tid,
                                          mpos=p2 if k == 0 else p1, isize=isize if k == 0 else -isize, tags={"RG": "g1" if f % 2 else "g2"}), f))
    seq, cigar = _read(targets["chrB"], 980 + shift, {1000 + shift: ("ins", "TT")})                      # the indel seen once
    records.append((1, dict(qname="once", flag=0, pos=980 + shift, mapq=60, cigar=cigar, seq=seq, qual=[30] * READ, mtid=-1, mpos=-1, isize=0, tags={"RG": "g1"}), 0))
    records.sort(key=lambda x: (x[0], x[1]["pos"]))
    refs = [(n, length) for n in names]
    bam = os.path.join(str(tmp), "discover.bam")
    _bamwriter.write_bam(bam, header, refs, [(t, r) for t, r, _ in records])
    bams = []
    for half in (0, 1):
        bams.append(os.path.join(str(tmp), "discover_pool%d.bam" % half))
        _bamwriter.write_bam(bams[-1], header, refs, [(t, r) for t, r, f in records if f % 2 == half])
    lst = os.path.join(str(tmp), "discover_bams.txt")
    open(lst, "w").write("".join(b + "\n" for b in bams))
    return dict(bam=bam, bams=bams, list=lst, fasta=fasta, targets=targets, names=names, records=records, shift=shift)


def discover_in_library(prefix, fasta, bam=None, bam_list=None, tid=None, region=None, min_dist=20, min_count=-1, max_count=-1, batch_candidates=0,
                        events_cap=0, host_convert=False, hook=cases.CHECKER_HOOK):
    """ddh_discover_windows: the discovery stage of dindel_gpu --discover; hook None = the device.  Returns the number of window lines;
    raises RuntimeError with the message the stage threw."""
    lib = hostlib.load()
    lib.ddh_discover_windows.restype = C.c_long
    lib.ddh_discover_windows.argtypes = [C.c_char_p] * 6 + [C.c_long] * 3 + [C.c_int] * 3 + [cases.HOOK_TYPE, C.c_void_p, C.c_char_p, C.c_int]
    err = C.create_string_buffer(1024)
    enc = lambda s: None if s is None else str(s).encode()
    n = lib.ddh_discover_windows(enc(bam), enc(bam_list), enc(tid), enc(region), enc(fasta), enc(prefix), min_dist, min_count, max_count, batch_candidates,
                                 events_cap, 1 if host_convert else 0, hook if hook is not None else cases.HOOK_TYPE(), None, err, len(err))
    if n < 0:
        raise RuntimeError(err.value.decode())
    return n
