"""dindel_haplotypes end to end on the synthetic BAM / window sample of tests/test_n2_driver_gpu.py: the block tables from the device
and from the host give the same W / R / H file, every window with a planted variant holds the reference haplotype and the planted one,
and the chain dindel_haplotypes -> dindel_hapalign -> dindel_gpu -> dindel_glf2vcf calls the planted variants without any haplotype file
from elsewhere.  (The .glf.txt is not compared with the one the sample's own haplotype file gives: that file holds two haplotypes per
window by construction, this one what the reads show.)"""
import os
import subprocess

import pytest

from tests.test_haplotypes_cpu import parse_wrh
from tests.test_n2_driver_gpu import HOST, run_driver, scene  # noqa: F401  (scene: the module-scoped sample)

pytestmark = pytest.mark.gpu


def _env():
    import torch
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return env


def test_chain_from_reads_to_vcf_without_a_haplotype_file(scene):  # noqa: F811
    tmp, ref = scene["tmp"], scene["ref"]
    dev, hst = str(tmp / "cand_dev.txt"), str(tmp / "cand_host.txt")
    base = [os.path.join(HOST, "dindel_haplotypes"), "--bamFile", scene["bam"], "--ref", scene["fasta"], "--varFile", scene["vf"]]
    r = subprocess.run(base + ["--outputFile", dev, "--batchWindows", "4"], env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "on the device" in r.stderr, r.stderr[-2000:]
    r2 = subprocess.run(base + ["--outputFile", hst, "--hostDistribution", "--quiet"], env=_env(), capture_output=True, text=True, timeout=120)
    assert r2.returncode == 0, r2.stderr[-2000:]
    assert open(dev, "rb").read() == open(hst, "rb").read()
    assert "too_few_reads" in r.stderr                         # the window without reads: one line, no record

    wins = {w["index"]: w for w in parse_wrh(open(dev).read())}
    assert sorted(wins) == [1, 2, 3, 4, 5]
    for wi, (left, kind, _) in enumerate(scene["spec"][:5], start=1):
        w = wins[wi]
        assert left <= w["left"] < left + 60 < w["right"] <= left + 120 and w["ref"] == ref[w["left"]:w["right"] + 1]
        planted = ref[w["left"]:left + 60] + ("GAT" + ref[left + 60:w["right"] + 1] if kind == "ins" else ref[left + 62:w["right"] + 1])
        assert w["ref"] in w["haps"] and planted in w["haps"], wi
        assert w["haps"] == sorted(set(w["haps"])) and 2 <= len(w["haps"]) <= 200

    aligned = str(tmp / "cand_aligned.txt")
    subprocess.check_call([os.path.join(HOST, "dindel_hapalign"), "--hapFile", dev, "--outputFile", aligned, "--quiet"], env=_env())
    glf, rows = run_driver(dict(scene, hf=aligned), "from_reads")
    assert sum(r["msg"] == "ok" for r in rows) >= 5
    lst, vcf = str(tmp / "from_reads_glfs.txt"), str(tmp / "from_reads.vcf")
    open(lst, "w").write(glf + "\n")
    subprocess.check_call([os.path.join(HOST, "dindel_glf2vcf"), "-i", lst, "-o", vcf, "-r", scene["fasta"], "-s", "S1"], stdout=subprocess.DEVNULL)
    body = {int(l[1]): l for l in (x.split("\t") for x in open(vcf).read().split("\n") if x and not x.startswith("#"))}
    for pos, gt in ((5060, "0/1:"), (5460, "0/1:"), (6260, "0/1:")):     # the heterozygous 2-bp deletions: REF 3 bases, ALT the anchor
        assert body[pos][3] == ref[pos - 1:pos + 2] and body[pos][4] == ref[pos - 1] and body[pos][9].startswith(gt), body[pos]
    assert body[5860][3] == ref[5859] and body[5860][4] == ref[5859] + "GAT" and body[5860][9].startswith("1/1:")      # the homozygous insertion
