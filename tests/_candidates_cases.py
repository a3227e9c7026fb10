"""TEST INFRASTRUCTURE ONLY: inputs shared by tests/test_candidates_cpu.py and tests/test_gpu_candidates.py — references with planted
repeats, candidate files, a synthetic BAM on three targets with two libraries, and the two ways to run the tool (the binary on the
device; candidatesMain inside the host library with the checker's alignments injected through the library's hook)."""
import ctypes as C
import os
import random
import subprocess

import numpy as np

from dindel_tgi_amd import capi, hostlib
from tests import _bamwriter, _hapalign_oracle as orc
from tests.test_glf_vcf_cpu import write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dindel_tgi_amd", "host", "dindel_candidates")

HOOK_TYPE = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(capi.dd_align_batch), C.POINTER(C.c_int32), C.POINTER(C.c_int16))
_cache = {}


def _checker_hook(_data, bp, status, ref_pos):
    """the library's AlignHook: statuses and offset slices from tests/_hapalign_oracle.py"""
    b = bp.contents
    roff = np.ctypeslib.as_array(C.cast(b.ref_off, C.POINTER(C.c_int32)), (b.n_refs + 1,))
    hoff = np.ctypeslib.as_array(C.cast(b.hap_off, C.POINTER(C.c_int32)), (b.n_pairs + 1,))
    pref = np.ctypeslib.as_array(C.cast(b.pair_ref, C.POINTER(C.c_int32)), (b.n_pairs,))
    refs, haps = C.string_at(b.ref_seq, int(roff[-1])), C.string_at(b.hap_seq, int(hoff[-1]))
    for i in range(b.n_pairs):
        r, h = refs[roff[pref[i]]:roff[pref[i] + 1]], haps[hoff[i]:hoff[i + 1]]
        if not r or not h:
            status[i] = capi.DD_ALIGN_EMPTY
        elif max(len(r), len(h)) > capi.DD_LONG_MAX_HAP_LEN:
            status[i] = capi.DD_ALIGN_TOO_LONG
        else:
            status[i] = capi.DD_ALIGN_OK
            if (r, h) not in _cache:
                _cache[(r, h)] = orc.align(r, h)[3]
            for k, v in enumerate(_cache[(r, h)].tolist()):
                ref_pos[int(hoff[i]) + k] = v
            continue
        for k in range(int(hoff[i]), int(hoff[i + 1])):
            ref_pos[k] = -1


CHECKER_HOOK = HOOK_TYPE(_checker_hook)


def run_in_library(args, hook=CHECKER_HOOK):
    """candidatesMain(args) inside libdindel_host.so with the alignments injected; returns the exit code"""
    lib = hostlib.load()
    lib.ddh_candidates_main.argtypes = [C.c_int, C.POINTER(C.c_char_p), HOOK_TYPE, C.c_void_p]
    argv = (C.c_char_p * (len(args) + 2))(b"dindel_candidates", *[str(a).encode() for a in args], None)
    return lib.ddh_candidates_main(len(args) + 1, argv, hook, None)


def run_tool(args):
    """the binary: (exit code, stdout, stderr)"""
    env = dict(os.environ)
    try:
        import torch
        env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    except ImportError:
        pass
    p = subprocess.run([TOOL] + [str(a) for a in args], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return p.returncode, p.stdout.decode(), p.stderr.decode()


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def repeat_reference(seed=3, n=20000):
    """(sequence, [(refpos, len, seq)]): a random reference with homopolymers and 2- / 3-mer repeats planted every 60 bases, and about 300
    candidates of length 1 ... 40: an insertion or deletion of whole units at every position of its repeat (so that several land on
    one canonical variant), random indels elsewhere, and the window switch at |len| = 33 / 34"""
    rng = random.Random(seed)
    s = list(rand_seq(rng, n))
    plants = []
    at = 400
    for k in range(60):
        unit = [rng.choice("ACGT"), rng.choice(["AC", "GT", "CA", "TG"]), rng.choice(["ACG", "TTG", "CAG"])][k % 3]
        reps = rng.randint(3, 9)
        s[at:at + len(unit) * reps] = unit * reps
        plants.append((at, unit, reps))
        at += 60 + len(unit) * reps
    ref = "".join(s)
    cands = []
    for k, (p, unit, reps) in enumerate(plants[:36]):
        units = 1 + k % 2
        for x in range(0, len(unit) * (reps - units) + 1, len(unit) if k % 4 else 1):
            if k % 3 == 2:
                cands.append((p + x, len(unit) * units, (unit * 3)[x % len(unit):][:len(unit) * units]))
            else:
                cands.append((p + x, -len(unit) * units, "D" * (len(unit) * units)))
    for ln in list(range(1, 41)) + [33, 34, 33, 34]:
        p = rng.randrange(5000, n - 500)
        if rng.random() < 0.5:
            cands.append((p, ln, rand_seq(rng, ln)))
        else:
            cands.append((p, -ln, "D" * ln))
    return ref, cands


def candidate_file_text(tid, cands, ref, one_based=False):
    """`tid pos variant # 1` lines (the format realignCandidates reads), one per candidate in the order given"""
    lines = []
    for p, ln, seq in cands:
        var = "+" + seq if ln > 0 else "-" + ref[p:p - ln]
        lines.append("%s %d %s # 1\n" % (tid, p + (1 if one_based else 0), var))
    return "".join(lines)


def bam_sample(tmp, name="sample", seed=11, n_reads=260):
    """A BAM on three targets with two libraries (one whose histogram is cut by its length), reads without RG, duplicates, QC-fail,
    improper pairs and mates on another target; every fifth read carries an indel in its CIGAR.  Returns dict(bam, fasta, header,
    names, targets, records)."""
    rng = random.Random(seed)
    names = ["chrA", "chrB", "chrC"]
    targets = {"chrA": rand_seq(rng, 3000), "chrB": "ACGT" * 30 + rand_seq(rng, 900) + "A" * 12 + rand_seq(rng, 600), "chrC": rand_seq(rng, 700)}
    fasta = os.path.join(str(tmp), name + ".fa")
    write_fasta(fasta, [(n, targets[n]) for n in names])
    header = "@HD\tVN:1.0\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, len(targets[n])) for n in names) + \
             "@RG\tID:g1\tLB:libOne\tSM:s\n@RG\tID:g2\tLB:libTwo\tSM:s\n@RG\tID:g3\tSM:s\n"
    records = []
    for tid, tname in enumerate(names):
        tlen = len(targets[tname])
        poss = sorted(rng.randrange(0, tlen - 120) for _ in range(n_reads // 3))
        for k, pos in enumerate(poss):
            read = targets[tname][pos:pos + 60]
            cigar = "60M"
            if k % 5 == 0:
                ln = rng.randint(1, 6)
                if k % 10 == 0:
                    ins = rand_seq(rng, ln) if k % 20 else targets[tname][pos + 30 - ln:pos + 30]
                    read, cigar = read[:30] + ins + read[30:60 - ln], "30M%dI%dM" % (ln, 30 - ln)
                else:
                    read, cigar = read[:25] + targets[tname][pos + 25 + ln:pos + 60 + ln], "25M%dD35M" % ln
            if k % 7 == 3:
                cigar, read = "4S" + cigar + "3H", "NNNN" + read
            flag = 1 | 2
            if k % 11 == 0:
                flag |= 1024
            if k % 13 == 0:
                flag |= 512
            if k % 6 == 1:
                flag &= ~2
            if k % 17 == 0:
                flag = 0
            mtid = tid if k % 9 else (tid + 1) % 3
            lib = k % 4
            isize = int(rng.gauss(300, 20)) if lib != 1 else rng.choice([150, 150, 151, 152, 30000])
            r = dict(qname="r%d_%d" % (tid, k), flag=flag, pos=pos, mapq=60, cigar=cigar, seq=read, qual=[30] * len(read), mtid=mtid,
                     mpos=pos + 200, isize=isize * (1 if k % 2 else -1))
            if lib < 3:
                r["tags"] = {"RG": ["g1", "g2", "g3"][lib]}
            records.append((tid, r))
    records.append((-1, dict(qname="un", flag=4, pos=-1, mapq=0, cigar="", seq="ACGT", qual=[20] * 4)))
    bam = os.path.join(str(tmp), name + ".bam")
    _bamwriter.write_bam(bam, header, [(n, len(targets[n])) for n in names], records)
    return dict(bam=bam, fasta=fasta, header=header, names=names, targets=targets, records=records)
