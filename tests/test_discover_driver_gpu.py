"""dindel_gpu --discover: from a BAM and a FASTA alone.  Acceptance is equality with the chain, file for file:

    dindel_candidates --analysis getCIGARindels ... ; dindel_windows -i ... --oneFile ... ; dindel_gpu --varFile ... --ref ... ; dindel_glf2vcf

on the sample of tests/_discover_cases.py (two targets of 2,000 bp, 50-bp mate pairs at about 20x in two read groups, eight implanted
indels), with every option of the stage passed to the chain's tools the same way.  Without a library file every window of a
2,000-base target is skipped by read selection in both (see tests/_discover_cases.py), so the equality of the called rows, of the VCF's
records and of the realigned BAMs is checked a second time on the same sample laid out on 6,000-base targets."""
import os
import subprocess

import pytest

from dindel_tgi_amd import hapalign
from tests import _discover_cases as dc
from tests.test_glf_vcf_cpu import GLF_COLUMNS

pytestmark = pytest.mark.gpu
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dindel_tgi_amd", "host")


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


@pytest.fixture(scope="module")
def short(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", HOST])
    tmp = tmp_path_factory.mktemp("discover_short")
    return dict(dc.sample(tmp), tmp=tmp)


@pytest.fixture(scope="module")
def long_(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", HOST])
    tmp = tmp_path_factory.mktemp("discover_long")
    return dict(dc.sample(tmp, length=6000, shift=3000), tmp=tmp)


def both_ways(s, name, bam_args=None, cand_args=(), window_args=(), loop_args=(), discover_args=None, vcf=False, use_libraries=False, region=None):
    """the chain and the one command with the same options -> ({suffix: bytes} of the chain, of the one command, the one command's stdout)"""
    tmp = s["tmp"]
    chain, one = str(tmp / (name + "_chain")), str(tmp / (name + "_one"))
    bam_args = bam_args or ["--bamFile", s["bam"]]
    region_args = ["--tid", region[0], "--region", region[1]] if region else []
    # (a region run of the candidate tool writes --outputFile itself, and no library file)
    tool("dindel_candidates", "--analysis", "getCIGARindels", *bam_args, *region_args, "--ref", s["fasta"], "--outputFile",
         chain + ".variants.txt" if region else chain, "--quiet", *cand_args)
    tool("dindel_windows", "-i", chain + ".variants.txt", "--oneFile", chain + ".windows.txt", "--quiet", *window_args)
    lib_chain = ["--libFile", chain + ".libraries.txt"] if use_libraries else []
    tool("dindel_gpu", *bam_args, "--varFile", chain + ".windows.txt", "--ref", s["fasta"], "--outputFile", chain, "--quiet", *lib_chain, *loop_args)
    if vcf:
        lst = chain + ".glfs.txt"
        open(lst, "w").write(chain + ".glf.txt\n")
        tool("dindel_glf2vcf", "-i", lst, "-o", chain + ".vcf", "-r", s["fasta"])
    extra = list(discover_args if discover_args is not None else list(cand_args) + list(window_args).copy())
    r = tool("dindel_gpu", "--discover", *bam_args, *region_args, "--ref", s["fasta"], "--outputFile", one, "--quiet", *extra, *loop_args,
             *(["--useLibraries"] if use_libraries else []), *(["--vcf", one + ".vcf"] if vcf else []))
    files = {}
    for prefix in (chain, one):
        d, base = os.path.split(prefix)
        files[prefix] = {f[len(base):]: read(os.path.join(d, f), "rb") for f in os.listdir(d) if f.startswith(base + ".") and not f.endswith(".glfs.txt")}
    return files[chain], files[one], r.stdout


def rows_of(glf):
    lines = glf.decode().split("\n")
    assert lines[0].split(" ") == GLF_COLUMNS
    return [dict(zip(GLF_COLUMNS, l.split(" "))) for l in lines[1:] if l]


def check_equal(want, got, suffixes):
    assert sorted(got) == sorted(want) and set(suffixes) <= set(got), (sorted(got), sorted(want))
    for suffix in want:
        assert got[suffix] == want[suffix], suffix


WHOLE = (".variants.txt", ".libraries.txt", ".windows.txt", ".glf.txt")


def test_discover_equals_the_four_commands(short):
    want, got, _ = both_ways(short, "plain", vcf=True)
    check_equal(want, got, WHOLE + (".vcf",))
    assert got[".windows.txt"].count(b"\n") == 8 and len(rows_of(got[".glf.txt"])) >= 8


def test_discover_equals_the_four_commands_where_windows_are_called(long_):
    want, got, _ = both_ways(long_, "plain", vcf=True)
    check_equal(want, got, WHOLE + (".vcf",))
    rows = rows_of(got[".glf.txt"])
    called = {int(r["index"]) for r in rows if r["msg"] == "ok" and r["analysis_type"] == "dip.map"}
    assert len(called) >= 6, [(r["index"], r["msg"]) for r in rows]
    body = [l.split("\t") for l in got[".vcf"].decode().split("\n") if l and not l.startswith("#")]
    assert {"chrA", "chrB"} == {l[0] for l in body} and any(l[0] == "chrA" and l[1] == "3900" and l[4].endswith("GAT") for l in body), body


@pytest.mark.parametrize("name,kw", [
    ("minDist25", dict(window_args=("-m", "25"), discover_args=("--minDist", "25"))),
    ("minCount2", dict(window_args=("--minCount", "2"), discover_args=("--minCount", "2"))),
    ("useLibraries", dict(use_libraries=True)),
    ("region", dict(region=("chrA", "1,100-1,600"))),
    ("pool", dict(region=("chrA", "0-2000"), bam_args="list")),
    ("faster", dict(loop_args=("--faster",))),
    ("realigned", dict(loop_args=("--outputRealignedBAM", "--deviceCigars"))),
    ("candidateOptions", dict(cand_args=("--batchCandidates", "3", "--eventsCap", "1", "--hostConvert"))),
], ids=lambda x: x if isinstance(x, str) else "")
def test_discover_with_options_equals_the_chain_with_the_same_options(short, name, kw):
    kw = dict(kw)
    if kw.get("bam_args") == "list":
        kw["bam_args"] = ["--bamFiles", short["list"]]
    want, got, _ = both_ways(short, name, **kw)
    check_equal(want, got, (".variants.txt", ".windows.txt", ".glf.txt") + (() if kw.get("region") else (".libraries.txt",)))
    lines = got[".windows.txt"].decode().split("\n")[:-1]
    if name == "minDist25":
        assert len(lines) == 7 and any(" 1500,-" in l and " 1521,-" in l for l in lines)
    if name == "minCount2":
        assert not any("+TT" in l for l in lines) and len(lines) < 8
    if name in ("region", "pool"):
        assert {l.split(" ")[0] for l in lines} == {"chrA"} and len(lines) == (3 if name == "region" else 5)


@pytest.mark.parametrize("name,kw", [
    ("realignedDeviceCigars", dict(loop_args=("--outputRealignedBAM", "--deviceCigars"))),
    ("realigned", dict(loop_args=("--outputRealignedBAM",))),
    ("faster", dict(loop_args=("--faster",))),
    ("useLibraries", dict(use_libraries=True)),
    ("minDist25minCount2", dict(window_args=("-m", "25", "--minCount", "2"), discover_args=("--minDist", "25", "--minCount", "2"))),
], ids=lambda x: x if isinstance(x, str) else "")
def test_options_where_windows_are_called(long_, name, kw):
    want, got, _ = both_ways(long_, "long_" + name, **kw)
    check_equal(want, got, WHOLE)
    assert any(r["msg"] == "ok" for r in rows_of(got[".glf.txt"]))
    ra = [f for f in got if f.startswith(".ra.")]
    assert (len(ra) >= 6) == name.startswith("realigned"), sorted(got)


def test_option_errors_and_the_unchanged_text_without_discover(short):
    base = ["--bamFile", short["bam"], "--outputFile", str(short["tmp"] / "err")]
    r = tool("dindel_gpu", "--discover", *base, "--ref", short["fasta"], "--hapFile", "h.txt", ok=False)
    assert r.returncode == 1 and r.stderr == "--discover builds the haplotypes in the run: --hapFile cannot be given with it\n"
    r = tool("dindel_gpu", "--discover", *base, ok=False)
    assert r.returncode == 1 and r.stderr == "Please specify --ref: --discover needs the reference FASTA\n"
    r = tool("dindel_gpu", *base, "--ref", short["fasta"], ok=False)
    assert r.returncode == 1 and r.stderr == "Please specify --varFile\n" and r.stdout == ""
    r = tool("dindel_gpu", "--discover", "--bamFiles", short["list"], "--outputFile", str(short["tmp"] / "err"), "--ref", short["fasta"], ok=False)
    assert r.returncode == 1 and "Can extract the full set of indels from only BAM file at a time." in r.stderr
    r = tool("dindel_gpu", "--discover", *base, "--ref", short["fasta"], "--tid", "chrA", "--region", "1-500", "--useLibraries", ok=False)
    assert r.returncode == 1 and "--useLibraries needs a whole-file run" in r.stderr
    r = tool("dindel_gpu", *base, "--varFile", "w.txt", "--hapFile", "h.txt", "--vcf", "o.vcf", ok=False)
    assert r.returncode == 1 and r.stderr == "Please specify --ref: --vcf needs the reference FASTA\n"
    assert "--discover" in tool("dindel_gpu", "--help").stdout


def test_stage_on_the_device_trips_no_guard(short):
    prefix = str(short["tmp"] / "inproc")
    n = dc.discover_in_library(prefix, short["fasta"], bam=short["bam"], hook=None)
    assert n == 8
    assert hapalign.last_launch()["guard_trips"] == 0 and hapalign.events_last_launch()["guard_trips"] == 0
    assert hapalign.events_last_launch()["pairs"] >= 1
