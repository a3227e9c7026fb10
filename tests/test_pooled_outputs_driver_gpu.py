"""dindel_gpu --doPooled to the end of the pooled workflow: --pooledVcf / --pooledGlf (the calls and their per-pool likelihoods, written in the
run) and --outputRealignedBAM without --doDiploid (every read on a haplotype realigned to the first haplotype with the largest
likelihood, DInDel.cpp:498-520).

The scene is the three-pool scene of tests/test_pooled_driver_gpu.py, rebuilt here with what the realigned BAMs need — the haplotypes' A
records — and a fourth window whose variant haplotype lacks its A record, so that getCIGAR throws behind the window's pooled lines.  The
realigned records are compared with getCIGAR (the host's, through its C hook) applied to the CPU oracle's alignments of the reads each
window selected, to the haplotype the CPU oracle's log-likelihoods pick."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from dindel_tgi_amd import capi, hostlib
from tests import _bamwriter as bw
from tests import _cigar_cases as cc
from tests import _oracle
from tests.test_glf_vcf_cpu import GLF_COLUMNS, write_fasta
from tests.test_n2_pools_cpu import DRIVER, _env

pytestmark = pytest.mark.gpu
HOST = os.path.dirname(DRIVER)
N_REF = 12000


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pooledout")
    rng = np.random.default_rng(2103)
    ref = "".join(rng.choice(list("ACGT"), N_REF))
    spec = [(5000, "planted"), (5400, "pool2_empty"), (5800, "short"), (6200, "no_a_record")]
    windows, fixture, recs, hap_ref = [], [], [[], [], []], {}
    rid = 0
    for wi, (left, kind) in enumerate(spec, start=1):
        right = left + 120
        hap0 = ref[left:right + 1]
        alt = ref[:left + 60] + ref[left + 62:]
        hap1 = hap0[:60] + hap0[62:]
        var = "-" + hap0[60:62]
        windows.append("20 %d %d %d,%s" % (left, right, left + 60, var))
        v1 = "V I 60 %s 60 61 59 60 60 61 59 60" % var
        # A records: every haplotype base's offset on the window's reference sequence
        hap_ref[wi] = [list(range(121)), list(range(60)) + list(range(62, 121))]
        a0, a1 = ("A " + " ".join(map(str, h)) for h in hap_ref[wi])
        if kind == "short":
            fixture += ["W %d %d %d" % (wi, left, right), "H ACG", "V I 60 *REF 60 60 60 60 60 60 60 60", "H " + hap1, v1]
        else:
            fixture += ["W %d %d %d" % (wi, left, right), "H " + hap0, a0, "V I 60 *REF 60 60 60 60 60 60 60 60", "H " + hap1, v1] + ([a1] if kind != "no_a_record" else [])
        for pool in range(3):
            if kind == "pool2_empty" and pool == 2:
                continue
            for _ in range(14 if pool else 24):
                from_alt = pool == 0 and rng.random() < 0.5
                p = int(rng.integers(left - 30, left + 45))
                cut = left + 60 - p
                seq, cigar = (alt[p:p + 100], "%dM2D%dM" % (cut, 100 - cut)) if from_alt else (ref[p:p + 100], "100M")
                recs[pool].append(dict(qname="q%04d" % rid, flag=int(rng.choice([0, 16])), pos=p, mapq=int(rng.choice([40, 50, 60])), cigar=cigar, seq=seq, qual=[30] * 100,
                                       mtid=-1, mpos=-1, isize=0, tags={}))
                rid += 1
    paths = []
    for pool in range(3):
        recs[pool].sort(key=lambda r: r["pos"])
        paths.append(str(tmp / ("pool%d.bam" % pool)))
        bw.write_bam(paths[-1], "@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:20\tLN:%d\n" % N_REF, [("20", N_REF)], [(0, r) for r in recs[pool]])
    lst, vf, hf, fasta = str(tmp / "bams.txt"), str(tmp / "windows.txt"), str(tmp / "haps.txt"), str(tmp / "ref.fa")
    open(lst, "w").write("\n".join(paths) + "\n")
    open(vf, "w").write("\n".join(windows) + "\n")
    open(hf, "w").write("\n".join(fixture) + "\n")
    write_fasta(fasta, [("20", ref)])
    subprocess.check_call(["make", "-s", "-C", HOST])
    return dict(tmp=tmp, ref=ref, paths=paths, list=lst, vf=vf, hf=hf, fasta=fasta, spec=spec, hap_ref=hap_ref, truth={r["qname"]: r for pool in recs for r in pool})


def run(cmd):
    r = subprocess.run([str(c) for c in cmd], env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert r.returncode == 0, (cmd, r.stderr[-2000:])
    return r


def run_driver(scene, prefix, *extra):
    out = str(scene["tmp"] / prefix)
    run([DRIVER, "--bamFiles", scene["list"], "--varFile", scene["vf"], "--hapFile", scene["hf"], "--outputFile", out, "--quiet", *extra])
    text = open(out + ".glf.txt").read()
    assert text.split("\n")[0].split(" ") == GLF_COLUMNS
    return out, text


def realigned_files(prefix):
    d, base = os.path.split(prefix)
    return {f[len(base):]: open(os.path.join(d, f), "rb").read() for f in os.listdir(d) if f.startswith(base + ".ra.")}


@pytest.fixture(scope="module")
def pooled_run(scene):
    return run_driver(scene, "pooled", "--doPooled")


def test_pooled_vcf_and_glf_written_in_the_run_equal_the_tools_run_afterwards(scene, pooled_run):
    tmp = scene["tmp"]
    vcf, glf = str(tmp / "run.vcf"), str(tmp / "run.called.txt")
    out, text = run_driver(scene, "withvcf", "--doPooled", "--ref", scene["fasta"], "--pooledVcf", vcf, "--pooledGlf", glf, "--numSamples", "3")
    assert text == pooled_run[1]                                                       # the .glf.txt itself is the one of the run without the new options
    lst, vcf_t, glf_t = str(tmp / "glfs.txt"), str(tmp / "tool.vcf"), str(tmp / "tool.called.txt")
    open(lst, "w").write(out + ".glf.txt\n")
    run([os.path.join(HOST, "dindel_pooled2vcf"), "-i", lst, "-o", vcf_t, "-r", scene["fasta"], "--numSamples", 3, "--numBamFiles", 3, "--quiet"])
    run([os.path.join(HOST, "dindel_pooled2glf"), "-g", lst, "-c", vcf_t, "-o", glf_t, "-b", scene["list"], "--quiet"])
    assert open(vcf).read() == open(vcf_t).read() and open(glf).read() == open(glf_t).read()
    data = [l.split("\t") for l in open(vcf).read().split("\n") if l and l[0] != "#"]
    # the planted deletion is called where pool 0 carries it; a called site has one likelihood line per pool, named by the run's BAM paths
    called = [l for l in data if l[6] == "PASS"]
    assert [int(l[1]) for l in called] == [left + 60 for left, kind in scene["spec"] if kind != "short"]
    assert all(l[0] == "20" and len(l[3]) == 3 and len(l[4]) == 1 for l in called)
    lines = [l.split(" ") for l in open(glf).read().split("\n")[:-1]]
    assert len(lines) >= 3 * len(called) and len(lines) % 3 == 0 and [l[6] for l in lines[:3]] == scene["paths"]
    assert {(l[0], int(l[1])) for l in lines} >= {("20", int(c[1])) for c in called}
    # --pooledVcf alone writes no likelihood file; --vcf beside it is independent: the diploid conversion finds no dip.map line
    vcf2, dipvcf = str(tmp / "alone.vcf"), str(tmp / "dip.vcf")
    run_driver(scene, "alone", "--doPooled", "--ref", scene["fasta"], "--pooledVcf", vcf2, "--numSamples", "3", "--vcf", dipvcf)
    assert open(vcf2).read() == open(vcf).read() and not [l for l in open(dipvcf).read().split("\n") if l and l[0] != "#"]


def oracle_windows(scene):
    """per computed window with all A records: the reads it selected, and per read (onHap, the haplotype of the first maximum, its hpos)"""
    lib = hostlib.load()
    lib.ddh_get_reads_pools_json.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_double, C.c_char_p,
                                             C.c_int, C.c_char_p, C.c_int]
    n = len(scene["spec"])
    win = (C.c_int * (2 * n))(*[x for left, _ in scene["spec"] for x in (left, left + 120)])
    prm = (C.c_int * 4)(10000, 500, 20, 0)
    out = C.create_string_buffer(1 << 24)
    assert lib.ddh_get_reads_pools_json("\n".join(scene["paths"]).encode(), b"", b"20", win, n, prm, 0.99, b"", 1, out, len(out)) > 0
    selected = json.loads(out.value.decode())
    p = capi.params_cli_defaults()
    res = {}
    for wi, (left, kind) in enumerate(scene["spec"], start=1):
        if kind in ("short", "no_a_record"):
            continue
        hap0 = scene["ref"][left:left + 121]
        haps = [hap0, hap0[:60] + hap0[62:]]
        reads = []
        for r in selected[wi - 1]["reads"]:
            pairs = [_oracle.pair(h, r[6], [1.0 - 10 ** -3.0] * len(r[6]), r[2], int(r[7]), left, p, unmapped=bool(r[5])) for h in haps]
            on_hap = any(not o.offHapHMQ for o, _ in pairs)
            best, llmax = 0, -np.inf
            for h, (o, _) in enumerate(pairs):                                         # strict `>` from -inf: the first of the largest
                if o.ll > llmax:
                    best, llmax = h, o.ll
            reads.append(dict(name=r[0], on_hap=on_hap, hap=best, hpos=pairs[best][1]))
        res[wi] = reads
    return res


def test_pooled_realigned_bams_carry_the_first_maximum_haplotypes_cigar(scene, pooled_run):
    out, text = run_driver(scene, "ra", "--doPooled", "--outputRealignedBAM")
    # window 4 wrote its pooled lines and then failed in getCIGAR: the skipped line follows them, as in the reference's catch
    lines = text.split("\n")
    assert [l for l in lines if not l.startswith("error_Haplotype_has_not_been_aligned!")] == pooled_run[1].split("\n")
    late = [i for i, l in enumerate(lines) if l.startswith("error_Haplotype_has_not_been_aligned!")]
    assert len(late) == 1 and lines[late[0]].split(" ")[1] == "4" and lines[late[0] - 1].split(" ")[1:3] == ["4", "singlevariant"]
    files = realigned_files(out)
    want_names = {".ra.%d_20_%d_%d.bam" % (wi, left + 20, left + 120 - 20) for wi, (left, kind) in enumerate(scene["spec"], start=1) if kind in ("planted", "pool2_empty")}
    assert set(files) == want_names                                                    # one per computed window; none for the skipped ones
    header0, refs0, _ = bw.read_bam(scene["paths"][0])
    oracle = oracle_windows(scene)
    moved = on = copied = 0
    for wi, reads in oracle.items():
        left = scene["spec"][wi - 1][0]
        header, refs, recs = bw.read_bam("%s.ra.%d_20_%d_%d.bam" % (out, wi, left + 20, left + 100))
        assert (header, refs) == (header0, refs0) and [r["qname"] for r in recs] == [r["name"] for r in reads]
        for got, want in zip(recs, reads):
            t = scene["truth"][got["qname"]]
            assert (got["seq"], got["qual"], got["flag"], got["mapq"], got["mpos"]) == (t["seq"], t["qual"], t["flag"], t["mapq"], t["mpos"])
            if not want["on_hap"]:
                assert (got["pos"], got["cigar"], got["isize"]) == (t["pos"], t["cigar"], t["isize"])       # copied
                copied += 1
                continue
            cig, ref_pos = cc.host_cigar(scene["hap_ref"][wi][want["hap"]], want["hpos"])
            pos = -1 if ref_pos < 0 else left + ref_pos
            assert (got["pos"], got["cigar"], got["isize"]) == (pos, "".join("%d%s" % (n, bw.CIGAR_OPS[op]) for op, n in cig), pos - t["mpos"]), (wi, got["qname"])
            on += 1
            moved += want["hap"] == 1
    assert on > 60 and moved >= 8                                                      # both haplotypes were chosen
    # the device's CIGARs, and every read through the host fallback (one operation kept per read): the same bytes
    assert realigned_files(run_driver(scene, "radev", "--doPooled", "--outputRealignedBAM", "--deviceCigars")[0]) == files
    tight, tight_text = run_driver(scene, "racap1", "--doPooled", "--outputRealignedBAM", "--deviceCigars", "--cigarOpsCap", "1")
    assert realigned_files(tight) == files and tight_text == text
    # --faster writes none, as before
    assert not realigned_files(run_driver(scene, "rafaster", "--doPooled", "--outputRealignedBAM", "--faster")[0])


def test_both_analyses_write_the_diploid_steps_bams(scene):
    """--doPooled --doDiploid --outputRealignedBAM: the diploid step's file has the pooled one's name and is the one that stays — the bytes
    of the run without --doPooled"""
    both = realigned_files(run_driver(scene, "raboth", "--doPooled", "--doDiploid", "--outputRealignedBAM")[0])
    dip = realigned_files(run_driver(scene, "radip", "--doDiploid", "--outputRealignedBAM")[0])
    assert both == dip and len(both) == 2
