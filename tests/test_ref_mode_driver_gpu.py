"""dindel_gpu --ref FASTA without --hapFile: each window's candidate haplotypes are built, aligned and annotated inside the run
(getHaplotypes, DInDel.cpp:1526-1645, and what empiricalDistributionMethod does with its result, :393-405).  On the sample of
tests/test_n2_driver_gpu.py the .glf.txt must equal what the three tools in a row give (dindel_haplotypes -> dindel_hapalign ->
dindel_gpu --hapFile), whichever way the stage is run; the windows getHaplotypes returns `true` for write no row, the strings it
throws become skipped lines and late skips (several pools: the writer's redo chain), realigned BAMs come out the same, and
dindel_glf2vcf calls the planted variants from the one command's output."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _bamwriter as bw
from tests.test_glf_vcf_cpu import GLF_COLUMNS, write_fasta
from tests.test_n2_driver_gpu import HOST, run_driver, scene  # noqa: F401  (scene: the module-scoped sample)

pytestmark = pytest.mark.gpu


def _env():
    import torch
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return env


def run_ref(scene, prefix, *extra, bam_args=None):  # noqa: F811
    """dindel_gpu --ref (no --hapFile) -> (the .glf.txt's text, stdout, stderr, output prefix)"""
    out = str(scene["tmp"] / prefix)
    r = subprocess.run([os.path.join(HOST, "dindel_gpu")] + (bam_args or ["--bamFile", scene["bam"]]) +
                       ["--varFile", scene["vf"], "--ref", scene["fasta"], "--outputFile", out, *extra], env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    text = open(out + ".glf.txt").read()
    assert text.split("\n")[0].split(" ") == GLF_COLUMNS
    return text, r.stdout, r.stderr, out


def rows_of(text):
    return [dict(zip(GLF_COLUMNS, l.split(" "))) for l in text.split("\n")[1:] if l]


@pytest.fixture(scope="module")
def chain(scene):  # noqa: F811
    """the three tools in a row, once: the haplotype file and the .glf.txt every --ref run is compared with"""
    tmp = scene["tmp"]
    cand, aligned = str(tmp / "chain_cand.txt"), str(tmp / "chain_aligned.txt")
    subprocess.check_call([os.path.join(HOST, "dindel_haplotypes"), "--bamFile", scene["bam"], "--ref", scene["fasta"], "--varFile", scene["vf"],
                           "--outputFile", cand, "--quiet"], env=_env(), stderr=subprocess.DEVNULL)
    subprocess.check_call([os.path.join(HOST, "dindel_hapalign"), "--hapFile", cand, "--outputFile", aligned, "--quiet"], env=_env())
    glf, _rows = run_driver(dict(scene, hf=aligned), "chain")
    return dict(aligned=aligned, glf=open(glf).read())


def test_ref_mode_equals_the_three_tools_in_a_row(scene, chain):  # noqa: F811
    text, stdout, stderr, _ = run_ref(scene, "ref_plain")
    want, got = rows_of(chain["glf"]), rows_of(text)
    # every window that is not skipped: the same rows, byte for byte
    ok_want = [l for l in chain["glf"].split("\n")[1:] if l and not l.startswith("error_")]
    ok_got = [l for l in text.split("\n")[1:] if l and not l.startswith("error_")]
    assert ok_got == ok_want and len(ok_got) >= 10
    assert sorted({int(r["index"]) for r in got if r["msg"] == "ok"}) == [1, 2, 3, 4, 5]
    # the window without reads: getReads throws before any haplotype is made, in both (DInDel.cpp:1362)
    assert [r["msg"] for r in got if r["index"] == "6"] == ["error_too_few_reads"] == [r["msg"] for r in want if r["index"] == "6"]
    # window 5 (a 3-base haplotype in the sample's own haplotype file, "hapSize error." there): getHaplotypes builds its haplotypes
    # from the reads and the 121-base reference like any other window's (DInDel.cpp:1530-1598), so it is called, not skipped
    w5 = [r for r in got if r["index"] == "5"]
    assert [r["msg"] for r in w5] == ["ok"] * len(w5) and any(r["analysis_type"] == "dip.map" and r["nref_all"].startswith("-") for r in w5)
    assert "no_haplotypes_for_this_window" not in text
    assert "windows: 6 skipped: 1" in stdout
    assert text == chain["glf"]                                # and here the skipped line is the same too


@pytest.mark.parametrize("extra", [("--hostConvert",), ("--hostDistribution",), ("--hostConvert", "--hostDistribution"), ("--batchWindows", "1"),
                                   ("--batchWindows", "4"), ("--prepareThreads", "1"), ("--prepareThreads", "3", "--batchWindows", "2")],
                         ids=lambda e: "".join(e).replace("--", "_"))
def test_ref_mode_option_variants_write_the_same_bytes(scene, chain, extra):  # noqa: F811
    text, _, _, _ = run_ref(scene, "ref_var" + "".join(extra).replace("--", "_"), "--quiet", *extra)
    assert text == chain["glf"]


def test_windows_getHaplotypes_passes_over_write_no_row(scene):  # noqa: F811
    """--skipMaxHap 1: every window with more than one combination leaves getHaplotypes at :1569 with `true` — a cerr line, no row in the
    table, no skipped window.  The window without reads is skipped by read selection as before."""
    text, stdout, stderr, _ = run_ref(scene, "ref_skipmax", "--skipMaxHap", "1")
    assert [(r["index"], r["msg"]) for r in rows_of(text)] == [("6", "error_too_few_reads")]
    assert "windows: 6 skipped: 1" in stdout
    assert stderr.count("too many haplotypes [>exp(") == 5 and stderr.count("SKIPPING!") == 5 and stderr.count("skipped 20 ") == 1
    assert re.search(r"tid: 20 pos: 5060 too many haplotypes \[>exp\([0-9.]+\)\]\ntid: 20 pos:  5060 SKIPPING!\n", stderr)


def test_hap_read_product_is_thrown_from_the_haplotypes_made(scene):  # noqa: F811
    """--maxHapReadProd 1: the product test of :1581 returns with the haplotypes still in place, so :395-399 throws."""
    text, stdout, stderr, _ = run_ref(scene, "ref_prod", "--maxHapReadProd", "1")
    rows = rows_of(text)
    assert [(r["index"], r["msg"]) for r in rows] == [(str(i), "error_skipped_numhap_times_numread>1") for i in range(1, 6)] + [("6", "error_too_few_reads")]
    assert "windows: 6 skipped: 6" in stdout and "SKIPPING!" not in stderr and stderr.count("too many haplotypes [>") == 5
    # a limit between the windows' products: those above are thrown, the others are called as in the plain run
    plain = run_ref(scene, "ref_prod0", "--quiet")[0].split("\n")
    n_reads = {int(l.split(" ")[1]): int(l.split(" ")[11]) for l in plain[1:] if " dip.map " in l}
    cut = sorted(n_reads.values())[2]
    # (an upper bound on every window's product that keeps windows with fewer reads: 200 haplotypes at most)
    text2 = run_ref(scene, "ref_prod2", "--quiet", "--maxHapReadProd", str(cut * 2 - 1))[0]
    msgs = {}
    for r in rows_of(text2):
        msgs.setdefault(int(r["index"]), set()).add(r["msg"])
    for wi, n in n_reads.items():
        if n >= cut:
            assert msgs[wi] == {"error_skipped_numhap_times_numread>%d" % (cut * 2 - 1)}, wi     # at least two haplotypes each


def test_realigned_bams_equal_the_chain(scene, chain):  # noqa: F811
    tmp = scene["tmp"]
    run_driver(dict(scene, hf=chain["aligned"]), "chain_ra", "--outputRealignedBAM")
    want = {f[len("chain_ra"):]: open(str(tmp / f), "rb").read() for f in os.listdir(str(tmp)) if f.startswith("chain_ra.ra.")}
    assert len(want) == 5
    for prefix, extra in (("ref_ra", ()), ("ref_rad", ("--deviceCigars",)), ("ref_rah", ("--hostConvert",))):
        text = run_ref(scene, prefix, "--quiet", "--outputRealignedBAM", *extra)[0]
        assert text == chain["glf"]
        got = {f[len(prefix):]: open(str(tmp / f), "rb").read() for f in os.listdir(str(tmp)) if f.startswith(prefix + ".ra.")}
        assert got == want, prefix


def test_hapfile_wins_over_ref(scene):  # noqa: F811
    plain = open(run_driver(scene, "both0")[0]).read()
    both = open(run_driver(scene, "both1", "--ref", scene["fasta"], "--maxHap", "2", "--hostConvert")[0]).read()
    assert plain == both and "error_hapSize_error." in both


def test_ref_mode_to_the_vcf(scene):  # noqa: F811
    tmp, ref = scene["tmp"], scene["ref"]
    run_ref(scene, "ref_vcf", "--quiet")
    lst, vcf = str(tmp / "ref_vcf_glfs.txt"), str(tmp / "ref_vcf.vcf")
    open(lst, "w").write(str(tmp / "ref_vcf.glf.txt") + "\n")
    subprocess.check_call([os.path.join(HOST, "dindel_glf2vcf"), "-i", lst, "-o", vcf, "-r", scene["fasta"], "-s", "S1"], stdout=subprocess.DEVNULL)
    body = {int(l[1]): l for l in (x.split("\t") for x in open(vcf).read().split("\n") if x and not x.startswith("#"))}
    for pos, gt in ((5060, "0/1:"), (5460, "0/1:"), (6260, "0/1:")):     # the heterozygous 2-bp deletions: REF 3 bases, ALT the anchor
        assert body[pos][3] == ref[pos - 1:pos + 2] and body[pos][4] == ref[pos - 1] and body[pos][9].startswith(gt), body[pos]
    assert body[5860][3] == ref[5859] and body[5860][4] == ref[5859] + "GAT" and body[5860][9].startswith("1/1:")      # the homozygous insertion


def test_thrown_haplotype_construction_is_a_late_skip_with_two_pools(tmp_path):
    """Two pools and windows holding a read whose CIGAR getHaplotypes throws on (a padding operation: "I don't know how to smoke this
    CIGAR", HaplotypeDistribution.cpp): the window gets the reference's skipped line, and the reference empties its read buffer behind it
    (DInDel.cpp:1401-1408), which the prepare stage could not know.  The writer's redo chain must make the output that of the loop run
    window by window."""
    rng = np.random.default_rng(5)
    n_ref = 30000
    ref = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, n_ref))
    fasta = str(tmp_path / "ref.fa")
    write_fasta(fasta, [("20", ref)])
    windows, left = [], 3000
    while left < n_ref - 3000:
        windows.append(left)
        left += int(rng.choice([60, 200, 400, 400, 900]))
    bad = [windows[3], windows[10], windows[11], windows[len(windows) // 2]]
    recs = [[], []]
    for k in range(9000):
        pos = int(rng.integers(100, n_ref - 300))
        L = int(rng.integers(60, 110))
        s = list(ref[pos:pos + L])
        if rng.random() < 0.3:
            j = int(rng.integers(0, L)); s[j] = "ACGT"[("ACGT".index(s[j]) + 1) % 4]
        cigar = "%dM" % L
        w = [x for x in windows if pos + 10 < x + 60 < pos + L - 10]
        if w and rng.random() < 0.4:                          # a 2-bp deletion in the middle of the window
            c = w[0] + 60 - pos
            s, cigar = list(ref[pos:pos + c] + ref[pos + c + 2:pos + L + 2]), "%dM2D%dM" % (c, L - c)
        recs[int(rng.integers(0, 2))].append(dict(qname="r%d" % k, flag=int(rng.choice([0, 16])), pos=pos, mapq=int(rng.choice([30, 40, 60])), cigar=cigar,
                                                  seq="".join(s), qual=[30] * len(s), mtid=-1, mpos=-1, isize=0, tags={}))
    for k, b in enumerate(bad):
        recs[k % 2].append(dict(qname="pad%d" % k, flag=0, pos=b + 10, mapq=60, cigar="40M5P60M", seq=ref[b + 10:b + 110], qual=[30] * 100, mtid=-1, mpos=-1,
                                isize=0, tags={}))
    paths = []
    for k in range(2):
        recs[k].sort(key=lambda r: r["pos"])
        paths.append(str(tmp_path / ("pool%d.bam" % k)))
        bw.write_bam(paths[-1], "@SQ\tSN:20\tLN:%d\n" % n_ref, [("20", n_ref)], [(0, r) for r in recs[k]])
    lst = str(tmp_path / "bams.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    vf = str(tmp_path / "windows.txt")
    open(vf, "w").write("".join("20 %d %d %d,-%s\n" % (x, x + 120, x + 60, ref[x + 60:x + 62]) for x in windows))
    subprocess.check_call(["make", "-s", "-C", HOST])
    s = dict(tmp=tmp_path, vf=vf, fasta=fasta)
    truth, _, err_truth, _ = run_ref(s, "wbw", "--windowByWindow", "--batchWindows", "16", "--prepareThreads", "2", bam_args=["--bamFiles", lst])
    thrown = "error_I_don't_know_how_to_smoke_this_CIGAR"
    by_lpos = {int(r["lpos"]): r["msg"] for r in rows_of(truth) if r["msg"].startswith("error_")}
    assert all(by_lpos.get(b) == thrown for b in bad), err_truth[-2000:]          # (a window 60 bases on sees the same read: it is thrown too)
    assert len(bad) <= truth.count(thrown) <= 2 * len(bad)
    assert sum(1 for r in rows_of(truth) if r["msg"] == "ok" and r["analysis_type"] == "dip.map") > len(windows) // 2
    for batch, threads in ((5, 3), (64, 2)):
        text, stdout, _, _ = run_ref(s, "b%d" % batch, "--batchWindows", str(batch), "--prepareThreads", str(threads), bam_args=["--bamFiles", lst])
        assert "re-prepared behind late skips" in stdout
        assert text == truth, "batches of %d windows" % batch
