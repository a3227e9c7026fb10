"""dindel_gpu --discover --candidateVCF on the device: indels that the sample's CIGARs do not show.

The sample (two 6,000-base targets, 50-bp mate pairs at about 20x; the pattern of tests/test_discover_driver_gpu.py, on the long targets
because read selection skips every window of a 2,000-base one, tests/_discover_cases.py) carries on chrA a haplotype with one unit less
of a CAG repeat and two inserted bases further on.  Every read cut from it has the CIGAR 50M: it lies where a mapper that never opens a
gap puts it, anchored by the longer of its two sides, the other side mismatching.  chrB has an ordinary deletion in the CIGARs (and an
insertion seen once), so that the run without known sites has something to call.

  * --discover alone writes no window on chrA and calls nothing there; with --candidateVCF naming the two sites — the deletion at a unit
    in the middle of its repeat — the realignment moves the deletion to the repeat's first unit, the windows cover both sites, the
    .glf.txt has their rows and --vcf reports both; the same with --vcfCandidatesOnly and with --faster.  (Without the feature the option
    is taken for a name with a value and ignored: the run is --discover alone, and these tests fail.)
  * every file of the run equals, byte for byte, the chain of the tools with the same options.
  * a 2,000-record VCF in planted repeats goes through dindel_vcf2candidates and realignCandidates: the device's events and
    --hostConvert write the same bytes, and no guard of the two launches trips."""
import os
import random
import subprocess

import pytest

from dindel_tgi_amd import hapalign
from tests import _bamwriter, _candidates_cases as cases, _discover_cases as dc
from tests.test_glf_vcf_cpu import GLF_COLUMNS, write_fasta

pytestmark = pytest.mark.gpu
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dindel_tgi_amd", "host")
READ, LENGTH = 50, 6000
REPEAT, UNITS, DEL_AT, INS_AT = 3000, 6, 3006, 3600   # (CAG)6 at 3000; the VCF names the unit at 3006; the insertion in front of base 3600
VCF_HEAD = '##fileformat=VCFv4.0\n##INFO=<ID=DP,Number=1,Type=Integer,Description="Total Depth">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n'


def _env():
    import torch
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return env


def tool(name, *args, ok=True):
    r = subprocess.run([os.path.join(HOST, name)] + [str(a) for a in args], env=_env(), capture_output=True, text=True, timeout=300)
    assert not ok or r.returncode == 0, (name, args, r.stderr[-3000:])
    return r


def read(path, mode="r"):
    with open(path, mode) as f:
        return f.read()


def other(c, k=1):
    return "ACGT"[("ACGT".index(c) + k) % 4]


def gapless(ref, hap, to_ref, h):
    """the read hap[h:h+READ] as a mapper that opens no gap places it: (reference position, sequence), the placement with fewer mismatches
    of the two that keep the read's first or its last base where the haplotype has it"""
    seq = hap[h:h + READ]
    best = None
    for start in (to_ref[h], to_ref[h + READ - 1] - (READ - 1)):
        if 0 <= start <= len(ref) - READ:
            mm = sum(a != b for a, b in zip(seq, ref[start:start + READ]))
            if best is None or mm < best[0]:
                best = (mm, start)
    return best[1], seq


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", HOST])
    tmp = tmp_path_factory.mktemp("known_sites")
    rng = random.Random(1909)
    A, B = list(dc._target(rng, LENGTH)), list(dc._target(rng, LENGTH))
    A[REPEAT:REPEAT + 3 * UNITS] = "CAG" * UNITS
    A[REPEAT - 1], A[REPEAT + 3 * UNITS] = "T", "T"          # the repeat ends on both sides; its first unit is the deletion's leftmost place
    ins = other(A[INS_AT - 1], 2) + other(A[INS_AT - 1])      # leftmost where it stands: the base in front is not its last letter
    for at in (3000, 1500):                                   # chrB's own deletion of B[3000:3002], and the known site at 1500, are leftmost as well
        if B[at - 1] == B[at + 1]:
            B[at - 1] = other(B[at + 1])
    A, B = "".join(A), "".join(B)
    hap = A[:DEL_AT] + A[DEL_AT + 3:INS_AT] + ins + A[INS_AT:]
    to_ref = list(range(DEL_AT)) + list(range(DEL_AT + 3, INS_AT)) + [INS_AT] * len(ins) + list(range(INS_AT, LENGTH))
    assert len(hap) == len(to_ref) == LENGTH - 1
    names = ["chrA", "chrB"]
    fasta = str(tmp / "known.fa")
    write_fasta(fasta, [("chrA", A), ("chrB", B)])
    header = "@HD\tVN:1.0\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, LENGTH) for n in names) + "@RG\tID:g1\tLB:libOne\tSM:s\n"
    records = []
    for f in range(LENGTH * 20 // (2 * READ)):
        isize = max(2 * READ + 10, int(rng.gauss(250, 15)))
        h1 = rng.randrange(0, len(hap) - isize - 12)
        (p1, s1), (p2, s2) = gapless(A, hap, to_ref, h1), gapless(A, hap, to_ref, h1 + isize - READ)
        for k, (p, seq, flag) in enumerate(((p1, s1, 99), (p2, s2, 147))):
            records.append((0, dict(qname="a%d" % f, flag=flag, pos=p, mapq=60, cigar="%dM" % READ, seq=seq, qual=[30] * READ, mtid=0, mpos=p2 if k == 0 else p1,
                                    isize=(p2 + READ - p1) * (1 if k == 0 else -1), tags={"RG": "g1"}), f))
        p1 = rng.randrange(0, LENGTH - isize - 12)
        p2 = p1 + isize - READ
        for k, (p, flag) in enumerate(((p1, 99), (p2, 147))):
            seq, cigar = dc._read(B, p, {3000: ("del", 2)})
            records.append((1, dict(qname="b%d" % f, flag=flag, pos=p, mapq=60, cigar=cigar, seq=seq, qual=[30] * READ, mtid=1, mpos=p2 if k == 0 else p1,
                                    isize=isize if k == 0 else -isize, tags={"RG": "g1"}), f))
    seq, cigar = dc._read(B, 3980, {4000: ("ins", other(B[3999]) * 2)})                                  # an indel seen once
    records.append((1, dict(qname="once", flag=0, pos=3980, mapq=60, cigar=cigar, seq=seq, qual=[30] * READ, mtid=-1, mpos=-1, isize=0, tags={"RG": "g1"}), 0))
    assert all(r["cigar"] == "50M" for t, r, _ in records if t == 0)
    records.sort(key=lambda x: (x[0], x[1]["pos"]))
    refs = [(n, LENGTH) for n in names]
    bam = str(tmp / "known.bam")
    _bamwriter.write_bam(bam, header, refs, [(t, r) for t, r, _ in records])
    bams = []
    for half in (0, 1):
        bams.append(str(tmp / ("known_pool%d.bam" % half)))
        _bamwriter.write_bam(bams[-1], header, refs, [(t, r) for t, r, f in records if f % 2 == half])
    lst = str(tmp / "known_bams.txt")
    open(lst, "w").write("".join(b + "\n" for b in bams))
    vcf = str(tmp / "sites.vcf")
    open(vcf, "w").write(VCF_HEAD + "chrA\t%d\t.\t%s\t%s\t50\tPASS\tDP=1\n" % (DEL_AT, A[DEL_AT - 1:DEL_AT + 3], A[DEL_AT - 1]) +
                         "chrA\t%d\t.\t%s\t%s\t.\tPASS\tDP=1\n" % (INS_AT, A[INS_AT - 1], A[INS_AT - 1] + ins))
    vcf2 = str(tmp / "more.vcf")                              # a second file: a site on chrB that no read supports
    open(vcf2, "w").write(VCF_HEAD + "chrB\t1500\t.\t%s\t%s\t50\tPASS\tDP=1\n" % (B[1499:1502], B[1499]))
    return dict(tmp=tmp, fasta=fasta, bam=bam, list=lst, vcf=vcf, vcf2=vcf2, A=A, B=B, ins=ins)


def rows_of(glf):
    lines = glf.decode().split("\n")
    assert lines[0].split(" ") == GLF_COLUMNS
    return [dict(zip(GLF_COLUMNS, l.split(" "))) for l in lines[1:] if l]


def files_of(prefix):
    d, base = os.path.split(prefix)
    return {f[len(base):]: read(os.path.join(d, f), "rb") for f in os.listdir(d) if f.startswith(base + ".") and not f.endswith(".glfs.txt")}


def one_command(s, name, vcfs, *extra, bam_args=None, region=None):
    one = str(s["tmp"] / (name + "_one"))
    region_args = ["--tid", region[0], "--region", region[1]] if region else []
    tool("dindel_gpu", "--discover", *(bam_args or ["--bamFile", s["bam"]]), *region_args, "--ref", s["fasta"], "--outputFile", one, "--quiet",
         *(["--candidateVCF", vcfs] if vcfs else []), "--vcf", one + ".vcf", *extra)
    return files_of(one)


def the_chain(s, name, vcfs, bam_args=None, region=None, only=False, min_count=None, loop_args=()):
    """dindel_candidates ; dindel_vcf2candidates ; dindel_candidates --analysis realignCandidates ; dindel_windows ; dindel_gpu --varFile --ref ; dindel_glf2vcf"""
    c = str(s["tmp"] / (name + "_chain"))
    bam_args = bam_args or ["--bamFile", s["bam"]]
    region_args = ["--tid", region[0], "--region", region[1]] if region else []
    kept = b""
    if not only:
        tool("dindel_candidates", "--analysis", "getCIGARindels", *bam_args, *region_args, "--ref", s["fasta"], "--outputFile", c + ".variants.txt" if region else c, "--quiet")
        kept = read(c + ".variants.txt", "rb")
        if min_count is not None:
            tool("dindel_windows", "-i", c + ".variants.txt", "--oneFile", c + ".scratch", "--selectedFile", c + ".selected", "--minCount", min_count, "--quiet")
            kept = read(c + ".selected", "rb")
            os.remove(c + ".scratch"), os.remove(c + ".selected")
    tool("dindel_vcf2candidates", "-i", vcfs, "-o", c + ".vcf.variants.txt", "-r", s["fasta"], "--quiet", *region_args)
    tool("dindel_candidates", "--analysis", "realignCandidates", "--varFile", c + ".vcf.variants.txt", "--ref", s["fasta"], "--outputFile", c + ".vcf.realigned", "--quiet")
    with open(c + ".candidates.txt", "wb") as f:
        f.write(kept + read(c + ".vcf.realigned.variants.txt", "rb"))
    tool("dindel_windows", "-i", c + ".candidates.txt", "--oneFile", c + ".windows.txt", "--quiet")
    tool("dindel_gpu", *bam_args, "--varFile", c + ".windows.txt", "--ref", s["fasta"], "--outputFile", c, "--quiet", *loop_args)
    lst = c + ".glfs.txt"
    open(lst, "w").write(c + ".glf.txt\n")
    tool("dindel_glf2vcf", "-i", lst, "-o", c + ".vcf", "-r", s["fasta"])
    return files_of(c)


KNOWN = (".vcf.variants.txt", ".vcf.realigned.variants.txt", ".candidates.txt", ".windows.txt", ".glf.txt", ".vcf")


def check_sites_are_called(s, got):
    """the two planted sites: moved, windowed, in the .glf.txt and in the VCF"""
    A, ins = s["A"], s["ins"]
    assert got[".vcf.variants.txt"].decode() == "chrA %d -CAG\nchrA %d +%s\n" % (DEL_AT, INS_AT, ins)
    assert got[".vcf.realigned.variants.txt"].decode() == "chrA %d -CAG # 1\nchrA %d +%s # 1\n" % (REPEAT, INS_AT, ins)        # the deletion has moved
    windows = [l.split(" ") for l in got[".windows.txt"].decode().split("\n") if l.startswith("chrA ")]
    assert [w[3:] for w in windows] == [["%d,-CAG" % REPEAT], ["%d,+%s" % (INS_AT, ins)]]
    assert int(windows[0][1]) <= REPEAT < REPEAT + 3 * UNITS <= int(windows[0][2]) and int(windows[1][1]) <= INS_AT <= int(windows[1][2])
    rows = [r for r in rows_of(got[".glf.txt"]) if r["tid"] == "chrA"]
    called = {(r["realigned_position"], r["nref_all"]) for r in rows if r["msg"] == "ok" and r["was_candidate_in_window"] == "1"}
    assert {(str(REPEAT), "-CAG"), (str(INS_AT), "+" + ins)} <= called, rows
    body = [l.split("\t") for l in got[".vcf"].decode().split("\n") if l and not l.startswith("#")]
    at = {(l[0], l[1]): l for l in body}
    assert at[("chrA", str(REPEAT))][3:5] == [A[REPEAT - 1:REPEAT + 3], A[REPEAT - 1]], body
    assert at[("chrA", str(INS_AT))][3:5] == [A[INS_AT - 1], A[INS_AT - 1] + ins], body
    return body


@pytest.fixture(scope="module")
def alone(sample):
    return one_command(sample, "alone", None)


@pytest.fixture(scope="module")
def both(sample):
    return one_command(sample, "both", sample["vcf"])


def test_discover_alone_does_not_see_the_gapless_indels(sample, alone):
    assert set(alone) == {".variants.txt", ".libraries.txt", ".windows.txt", ".glf.txt", ".vcf"}
    own = alone[".variants.txt"].decode().split("\n")[:-1]
    assert len(own) == 2 and own[0].startswith("chrB 3000 -%s # " % sample["B"][3000:3002]) and own[1] == "chrB 4000 +%s # 1" % (other(sample["B"][3999]) * 2)
    assert not any(l.startswith("chrA") for l in alone[".windows.txt"].decode().split("\n"))
    assert not [r for r in rows_of(alone[".glf.txt"]) if r["tid"] == "chrA"]
    body = [l.split("\t") for l in alone[".vcf"].decode().split("\n") if l and not l.startswith("#")]
    assert ["chrB", "3000"] in [l[:2] for l in body] and not [l for l in body if l[0] == "chrA"], body


def test_known_sites_are_realigned_windowed_and_called(sample, both):
    assert set(both) == set(KNOWN) | {".variants.txt", ".libraries.txt"}
    body = check_sites_are_called(sample, both)
    assert ["chrB", "3000"] in [l[:2] for l in body]                                                       # and the sample's own call is still there


def test_known_sites_alone_and_in_the_faster_model(sample, both):
    only = one_command(sample, "only", sample["vcf"], "--vcfCandidatesOnly")
    assert set(only) == set(KNOWN)
    body = check_sites_are_called(sample, only)
    assert {l[0] for l in body} == {"chrA"}
    faster = one_command(sample, "faster", sample["vcf"], "--faster")
    check_sites_are_called(sample, faster)
    for suffix in (".vcf.variants.txt", ".vcf.realigned.variants.txt", ".candidates.txt", ".windows.txt"):
        assert faster[suffix] == both[suffix]


@pytest.mark.parametrize("name", ["both", "only", "minCount2", "region", "pool"])
def test_one_command_equals_the_chain_byte_for_byte(sample, both, name):
    s = sample
    if name == "both":
        got, want = both, the_chain(s, name, s["vcf"])
    elif name == "only":
        got, want = one_command(s, "only_eq", s["vcf"], "--vcfCandidatesOnly", "--hostConvert"), the_chain(s, name, s["vcf"], only=True, loop_args=("--hostConvert",))
    elif name == "minCount2":
        got, want = one_command(s, name, s["vcf"], "--minCount", "2"), the_chain(s, name, s["vcf"], min_count=2)
        assert b" 4000 +" in both[".candidates.txt"] and b" 4000 +" not in got[".candidates.txt"] and got[".candidates.txt"].endswith(both[".vcf.realigned.variants.txt"])
    elif name == "region":
        vcfs, region = s["vcf"] + "," + s["vcf2"], ("chrA", "3,500-4,000")
        got, want = one_command(s, name, vcfs, region=region), the_chain(s, name, vcfs, region=region)
        assert got[".vcf.variants.txt"].decode() == "chrA %d +%s\n" % (INS_AT, s["ins"]) and got[".windows.txt"].count(b"\n") == 1
    else:
        vcfs, region, bam_args = s["vcf"] + "," + s["vcf2"], ("chrB", "0-6000"), ["--bamFiles", s["list"]]
        got, want = one_command(s, name, vcfs, bam_args=bam_args, region=region), the_chain(s, name, vcfs, bam_args=bam_args, region=region)
        assert got[".vcf.variants.txt"].decode() == "chrB 1500 -%s\n" % s["B"][1500:1502] and b"1500,-" in got[".windows.txt"] and b"3000,-" in got[".windows.txt"]
    expected = set(KNOWN) | (set() if name == "only" else {".variants.txt"}) | ({".libraries.txt"} if name in ("both", "minCount2") else set())
    assert set(got) == set(want) == expected, (sorted(got), sorted(want))
    for suffix in want:
        assert got[suffix] == want[suffix] and (got[suffix] or suffix == ".variants.txt"), suffix


def test_two_thousand_records_in_repeats_device_events_equal_host_convert(tmp_path):
    ref, cands = cases.repeat_reference()
    rng = random.Random(5)
    while len(cands) < 2000:
        p, ln = rng.randrange(200, len(ref) - 200), rng.randint(1, 6)
        cands.append((p, ln, cases.rand_seq(rng, ln)) if rng.random() < 0.5 else (p, -ln, "D" * ln))
    fasta, vcf = str(tmp_path / "rep.fa"), str(tmp_path / "rep.vcf")
    write_fasta(fasta, [("chrR", ref)])
    with open(vcf, "w") as f:
        f.write(VCF_HEAD)
        for p, ln, seq in cands:
            f.write("chrR\t%d\t.\t%s\t%s\t50\tPASS\tDP=1\n" % ((p, ref[p - 1], ref[p - 1] + seq) if ln > 0 else (p, ref[p - 1:p - ln], ref[p - 1])))
    out = str(tmp_path / "rep.variants.txt")
    tool("dindel_vcf2candidates", "-i", vcf, "-o", out, "-r", fasta)
    assert read(out) == "".join("chrR %d %s\n" % (p, "+" + seq if ln > 0 else "-" + ref[p:p - ln]) for p, ln, seq in cands)
    device = cases.HOOK_TYPE()                                                                             # NULL: the device aligns
    host, dev = str(tmp_path / "host"), str(tmp_path / "dev")
    args = ["--analysis", "realignCandidates", "--varFile", out, "--ref", fasta, "--quiet"]
    assert cases.run_in_library(args + ["--outputFile", host, "--hostConvert"], hook=device) == 0
    assert hapalign.last_launch()["guard_trips"] == 0
    assert cases.run_in_library(args + ["--outputFile", dev], hook=device) == 0
    assert hapalign.last_launch()["guard_trips"] == 0 and hapalign.events_last_launch()["guard_trips"] == 0 and hapalign.events_last_launch()["pairs"] >= 1
    assert read(dev + ".variants.txt") == read(host + ".variants.txt") and read(dev + ".variants.txt").count("\n") > 1000
