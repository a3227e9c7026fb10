"""dindel_gpu --doDiploid --outputRealignedBAM --deviceRealignDiploid: the device picks and certifies every window's most likely haplotype
pair and realigns each read by the diploid rule; one CIGAR per read comes back.  Every realigned BAM and the .glf.txt must be the bytes of
the run without the switch and of the run with --deviceCigars, whatever the batching and the cap; no alignment comes back; --checkDevicePair
finds no certified window whose pair the host would choose differently; and the one window made to tie is the only one left to the host.

The scene follows tests/test_n2_driver_gpu.py's: 24 windows with a planted 2-bp deletion or 3-bp insertion (heterozygous or homozygous),
then one window whose two candidate haplotypes (beside the reference) are the same sequence with the same records and whose reads all come from
them (equal likelihoods for every read, equal priors: the three best pairs tie exactly), one whose reference haplotype is too short (a late skip), one whose reads are random sequence (on no haplotype) and one
without reads."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _bamwriter as bw
from tests.test_glf_vcf_cpu import GLF_COLUMNS
from tests.test_n2_pools_cpu import DRIVER, _env

pytestmark = pytest.mark.gpu
HOST = os.path.dirname(DRIVER)
N_REF = 24000
N_PLANTED = 24
SWITCH = ("--deviceRealignDiploid", "--checkDevicePair")


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("diprealign")
    rng = np.random.default_rng(2310)
    r = list(rng.choice(list("ACGT"), N_REF))
    for i in range(3, len(r)):                     # no homopolymer longer than 3
        if r[i] == r[i - 1] == r[i - 2] == r[i - 3]:
            r[i] = "ACGT"[("ACGT".index(r[i]) + 1 + i % 3) % 4]
    ref = "".join(r)
    spec = [(5000 + 400 * i, "ins" if i % 3 == 2 else "del", 1.0 if i % 4 == 3 else 0.5) for i in range(N_PLANTED)]
    spec += [(5000 + 400 * N_PLANTED, "tie", 1.0), (5400 + 400 * N_PLANTED, "short", 0.5), (5800 + 400 * N_PLANTED, "junk", 0.0),
             (6200 + 400 * N_PLANTED, "empty", 0.0)]
    windows, fixture, recs = [], [], []
    rid = 0
    ref_rec = "V I 60 *REF 60 60 60 60 60 60 60 60"
    for wi, (left, kind, frac) in enumerate(spec, start=1):
        right = left + 120
        hap0 = ref[left:right + 1]
        a0 = "A " + " ".join(map(str, range(121)))
        if kind == "ins":
            insseq = "GAT"
            alt = ref[:left + 60] + insseq + ref[left + 60:]
            hap1 = hap0[:60] + insseq + hap0[60:]
            var = "+" + insseq
            v1 = "V I 60 %s 60 60 60 62 60 60 59 63" % var
            a1 = "A " + " ".join(map(str, list(range(60)) + [-1, -1, -1] + list(range(60, 121))))
        else:
            alt = ref[:left + 60] + ref[left + 62:]
            hap1 = hap0[:60] + hap0[62:]
            var = "-" + hap0[60:62]
            v1 = "V I 60 %s 60 61 59 60 60 61 59 60" % var
            a1 = "A " + " ".join(map(str, list(range(60)) + list(range(62, 121))))
        windows.append("20 %d %d %d,%s" % (left, right, left + 60, var))
        if kind == "short":
            fixture += ["W %d %d %d" % (wi, left, right), "H ACG", ref_rec, "H " + hap1, v1]
        elif kind == "tie":                        # the variant haplotype twice, record for record
            fixture += ["W %d %d %d" % (wi, left, right), "H " + hap0, a0, ref_rec, "H " + hap1, v1, a1, "H " + hap1, v1, a1]
        else:
            fixture += ["W %d %d %d" % (wi, left, right), "H " + hap0, a0, ref_rec, "H " + hap1, v1, a1]
        if kind == "empty":
            continue
        for _ in range(30):
            from_alt = rng.random() < frac
            p = int(rng.integers(left, left + 20)) if kind == "tie" else int(rng.integers(left - 60, left + 75))   # the tie window's reads lie inside the variant haplotype
            cigar = "100M"
            if kind == "junk":
                seq = "".join(rng.choice(list("ACGT"), 100))
            elif from_alt:
                cut = left + 60 - p
                if cut <= 0:
                    continue
                seq = alt[p:p + 100]
                if kind == "ins":
                    cigar = "100M" if cut >= 97 else "%dM3I%dM" % (cut, 97 - cut)
                else:
                    cigar = "100M" if cut >= 100 else "%dM2D%dM" % (cut, 100 - cut)
            else:
                seq = ref[p:p + 100]
            s = list(seq)
            if kind != "tie" and rng.random() < 0.1:
                k = int(rng.integers(0, 100)); s[k] = "ACGT"[("ACGT".index(s[k]) + 1) % 4]
            recs.append(dict(qname="q%04d" % rid, flag=int(rng.choice([0, 16])), pos=p, mapq=60, cigar=cigar, seq="".join(s), qual=[30] * 100,
                             mtid=-1, mpos=-1, isize=0, tags={}))
            rid += 1
    recs.sort(key=lambda r: r["pos"])
    bam = str(tmp / "reads.bam")
    bw.write_bam(bam, "@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:20\tLN:%d\n" % N_REF, [("20", N_REF)], [(0, r) for r in recs])
    vf, hf = str(tmp / "windows.txt"), str(tmp / "haps.txt")
    open(vf, "w").write("\n".join(windows) + "\n")
    open(hf, "w").write("\n".join(fixture) + "\n")
    subprocess.check_call(["make", "-s", "-C", HOST])
    return dict(tmp=tmp, bam=bam, vf=vf, hf=hf, spec=spec, tie=N_PLANTED + 1)


def run_driver(scene, prefix, *extra):
    out = str(scene["tmp"] / prefix)
    cmd = [DRIVER, "--bamFile", scene["bam"], "--varFile", scene["vf"], "--hapFile", scene["hf"], "--outputFile", out, "--quiet", "--timing",
           "--doDiploid", "--outputRealignedBAM", *extra]
    r = subprocess.run([str(c) for c in cmd], env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert r.returncode == 0, (cmd, r.stdout[-1000:], r.stderr[-2000:])
    text = open(out + ".glf.txt").read()
    assert text.split("\n")[0].split(" ") == GLF_COLUMNS
    timing = [l for l in r.stdout.split("\n") if l.startswith("timing:")]
    assert len(timing) == 1
    d, base = os.path.split(out)
    files = {f[len(base):]: open(os.path.join(d, f), "rb").read() for f in os.listdir(d) if f.startswith(base + ".ra.")}
    return files, text, dict(re.findall(r"(\w+)=(\S+)", timing[0]))


@pytest.fixture(scope="module")
def plain(scene):
    return run_driver(scene, "plain")


def test_same_files_as_without_the_switch_and_as_with_device_cigars(scene, plain):
    files, text, timing = plain
    have = {int(k[4:].split("_")[0]) for k in files}                                # ".ra.<index>_<tid>_<left>_<right>.bam"
    print("windows with a realigned BAM:", sorted(have))
    # the planted windows and the tie; not the late skip, not the window without reads (the window of random reads: whatever the run without the switch does)
    assert set(range(1, N_PLANTED + 2)) <= have <= set(range(1, N_PLANTED + 2)) | {N_PLANTED + 3} and int(timing["hpos_bytes"]) > 0
    for k in ("realign_bytes", "pair_uncertified", "pair_fallback_reads", "pair_disagreements"):
        assert k not in timing
    lines = text.split("\n")
    assert sum(l.startswith("error_hapSize_error.") for l in lines) == 1           # the late skip is in the picture
    got_files, got_text, got = run_driver(scene, "dip", *SWITCH)
    assert got_files == files and got_text == text
    assert int(got["hpos_bytes"]) == 0 and int(got["cigar_bytes"]) == 0 and int(got["realign_bytes"]) > 0
    assert int(got["pair_disagreements"]) == 0
    assert int(got["pair_uncertified"]) == 1                                       # the window made to tie, and no more
    assert int(got["pair_fallback_reads"]) == 0 and int(got["cigar_host_fallbacks"]) == 0
    assert int(got["fallback_hpos_bytes"]) > 0                                     # the tie window's alignments, recomputed for the host's CIGARs
    dev_files, dev_text, dev = run_driver(scene, "cigars", "--deviceCigars")
    assert dev_files == files and dev_text == text and "pair_uncertified" not in dev and int(dev["cigar_bytes"]) > int(got["realign_bytes"])
    both_files, both_text, both = run_driver(scene, "both", *SWITCH, "--deviceCigars")            # the switch wins over --deviceCigars beside it
    assert both_files == files and both_text == text and int(both["cigar_bytes"]) == 0 and both["realign_bytes"] == got["realign_bytes"]
    off_files, off_text, off = run_driver(scene, "noswitch", "--deviceRealignDiploid")      # without the check: no such count
    assert off_files == files and off_text == text and "pair_disagreements" not in off and int(off["pair_uncertified"]) == 1


@pytest.mark.parametrize("extra", [("--batchWindows", "1"), ("--windowByWindow",)])
def test_batching_does_not_change_the_bytes(scene, plain, extra):
    got_files, got_text, got = run_driver(scene, "b" + extra[0][2:], *SWITCH, *extra)
    assert got_files == plain[0] and got_text == plain[1]
    assert int(got["hpos_bytes"]) == 0 and int(got["pair_disagreements"]) == 0 and int(got["pair_uncertified"]) == 1


def test_a_cap_of_one_sends_the_longer_cigars_through_the_host(scene, plain):
    """As many reads go through the host as chosen CIGARs of the certified windows have more than one operation: the count of --deviceCigars at
    the same cap (every read of every window gets a CIGAR in the diploid step) less the tie window's, which is the host's as a whole.  The
    tie window's reads lie on its haplotypes, so its realigned BAM of the run without any switch holds their chosen CIGARs."""
    files, text, _ = plain
    left = scene["spec"][scene["tie"] - 1][0]
    tie_recs = bw.read_bam("%s.ra.%d_20_%d_%d.bam" % (str(scene["tmp"] / "plain"), scene["tie"], left + 20, left + 120 - 20))[2]
    tie_longer = sum(len(bw.parse_cigar(r["cigar"])) > 1 for r in tie_recs)
    assert len(tie_recs) >= 20 and tie_longer > 0
    ref_files, ref_text, ref = run_driver(scene, "cap1cig", "--deviceCigars", "--cigarOpsCap", "1")
    assert ref_files == files and ref_text == text and int(ref["cigar_host_fallbacks"]) > 0
    got_files, got_text, got = run_driver(scene, "cap1", *SWITCH, "--cigarOpsCap", "1")
    assert got_files == files and got_text == text
    assert int(got["pair_fallback_reads"]) == int(ref["cigar_host_fallbacks"]) - tie_longer > 0 and int(got["hpos_bytes"]) == 0
    assert int(got["pair_disagreements"]) == 0 and int(got["pair_uncertified"]) == 1
