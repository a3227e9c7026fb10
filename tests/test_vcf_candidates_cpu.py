"""Candidate indels from a VCF (host/vcf_candidates.cpp, dindel_vcf2candidates, dindel_gpu --discover --candidateVCF) without a GPU.

What the conversion writes is pinned against tests/golden/vcf_candidates.json, which tests/golden/make_vcf_candidates_fixtures.py
recorded from the reference's own python/convertVCFToDindel.py and python/utils/Variant.py: a NameError's text is compared exactly,
any other exception of the script by the fact that the conversion dies and by its type.  The discovery stage with known sites runs
with the checker's alignments injected through the library's hook, as tests/test_discover_cpu.py runs it, and every file it writes must
be the bytes of the tools (inside the library) run one after the other."""
import ctypes as C
import gzip
import json
import os
import re
import subprocess

import pytest

from dindel_tgi_amd import hostlib, vcf_candidates as vc
from tests import _candidates_cases as cases, _discover_cases as dc
from tests.test_glf_vcf_cpu import write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dindel_tgi_amd", "host")
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "vcf_candidates.json")))
# Python 2 names -> what Python 3, which recorded the fixtures, calls the same exception
PY3_TYPE = {"IOError": "OSError"}


@pytest.fixture(scope="module", autouse=True)
def built():
    hostlib.load()
    if not os.path.exists(os.path.join(HOST, "dindel_vcf2candidates")):
        subprocess.check_call(["make", "-s", "-C", HOST])


def run_tool(name, args):
    env = dict(os.environ)
    try:
        import torch
        env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    except ImportError:
        pass
    return subprocess.run([os.path.join(HOST, name)] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=120)


def read(path, mode="r"):
    with open(path, mode) as f:
        return f.read()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    d = tmp_path_factory.mktemp("vcfref")
    fa = str(d / "ref.fa")
    open(fa, "w").write(GOLD["fasta"])
    open(fa + ".fai", "w").write(GOLD["fai"])
    return fa


def write_case(tmp, case):
    names = []
    for k, text in enumerate(case["vcfs"]):
        names.append(str(tmp / ("%s_%d.vcf" % (case["name"], k))))
        with open(names[-1], "w", newline="") as f:
            f.write(text)
    return names


def died_as(thrown, error):
    """the thrown text against the recorded exception: a NameError's text exactly, any other by its type"""
    if error["type"] == "NameError":
        return thrown == error["text"]
    kind = thrown.split(":")[0]
    return PY3_TYPE.get(kind, kind) == error["type"]


# ---------------------------------------------------------------- Variant4
def test_variant4_table_from_the_script():
    assert len(GOLD["variant4"]) > 580
    bad = []
    for r, a, typ, off, s in GOLD["variant4"]:
        try:
            got = vc.variant4(r, a)
        except ValueError as e:
            got = (None, None, str(e))
        if got != (typ, off, s):
            bad.append((r, a, got, (typ, off, s)))
    assert not bad, bad[:10]


def test_variant4_values_named_in_the_header():
    for (r, a), want in {("AT", "A"): (1, "-T"), ("ACCCT", "AT"): (1, "-CCC"), ("TC", "TTTC"): (1, "+TT"), ("ACG", "ATCG"): (1, "+T"), ("AG", "ACCG"): (1, "+CC"),
                         ("ACGT", "AT"): (1, "-CG")}.items():
        assert vc.variant4(r, a)[1:] == want
    for r, a in (("A", "TA"), ("AC", "GTC"), ("AAC", "C")):
        with pytest.raises(ValueError, match="Don't think this is a proper VCF4 insertion"):
            vc.variant4(r, a)


# ---------------------------------------------------------------- whole conversions
@pytest.mark.parametrize("case", GOLD["conversions"], ids=lambda c: c["name"])
def test_conversion_in_the_library_and_by_the_tool(case, ref, tmp_path):
    names = write_case(tmp_path, case)
    out_l, out_t = str(tmp_path / "lib.txt"), str(tmp_path / "tool.txt")
    got = vc.convert_with_notes(names, ref, out_l, min_qual=case["minQual"])
    r = run_tool("dindel_vcf2candidates", ["-i", ",".join(names), "-o", out_t, "-r", ref, "--minQual", repr(case["minQual"])])
    if "error" in case:
        assert "throw" in got and died_as(got["throw"], case["error"]), (got, case["error"])
        assert got["stdout"] == case["stdout"]
        assert r.returncode == 1 and r.stderr.endswith("An error occurred!\n" + got["throw"] + "\n") and r.stdout == case["stdout"]
    else:
        assert "throw" not in got, got
        assert read(out_l) == "".join(l + "\n" for l in case["lines"]) and got["lines"] == len(case["lines"])
        assert got["stderr"] == case["stderr"] and got["stdout"] == case["stdout"]
        assert r.returncode == 0 and read(out_t) == read(out_l) and r.stderr == case["stderr"] and r.stdout == case["stdout"]


def test_fixture_holds_the_cases_the_rules_need():
    names = {c["name"] for c in GOLD["conversions"]}
    assert {"multi_alt", "qual_minQual_10", "ref_mismatch", "two_files", "blank_line_in_the_middle", "short_line", "one_field_short_of_the_last_column", "v3_header",
            "incomplete_description", "missing_main_column", "missing_fileformat", "sample_columns", "variant4_error_in_the_middle", "unknown_target"} <= names
    by = {c["name"]: c for c in GOLD["conversions"]}
    assert by["blank_line_in_the_middle"]["lines"] == ["chr1 20 -AC"] and by["short_line"]["lines"] == ["chr1 20 -AC"]     # the file's conversion ends there
    assert len(by["ref_mismatch"]["lines"]) == 4 and by["ref_mismatch"]["stderr"] == "REFSEQ inconsistency\n" * 3          # still written
    assert [l.split(" ")[1] for l in by["qual_minQual_10"]["lines"]] == ["20", "40", "50", "60"]                            # `.`, the boundary, above it


def test_gz_gives_the_bytes_of_the_plain_file(ref, tmp_path):
    case = [c for c in GOLD["conversions"] if c["name"] == "plain"][0]
    plain = write_case(tmp_path, case)[0]
    text = read(plain, "rb")
    one, members = str(tmp_path / "one.vcf.gz"), str(tmp_path / "members.vcf.gz")
    with gzip.open(one, "wb") as f:
        f.write(text)
    cut = [0, 40, 41, len(text) // 2, len(text)]
    with open(members, "wb") as f:                     # one gzip member per piece, as bgzip writes one per block, and its empty last member
        for a, b in zip(cut, cut[1:]):
            f.write(gzip.compress(text[a:b]))
        f.write(gzip.compress(b""))
    outs = []
    for k, src in enumerate((plain, one, members, plain + "," + members)):
        outs.append(str(tmp_path / ("out%d.txt" % k)))
        assert vc.convert(src, ref, outs[-1]) == len(case["lines"]) * (2 if "," in src else 1)
    assert read(outs[0]) == read(outs[1]) == read(outs[2]) == "".join(l + "\n" for l in case["lines"]) and read(outs[3]) == read(outs[0]) * 2
    with open(str(tmp_path / "cut.vcf.gz"), "wb") as f:
        f.write(read(one, "rb")[:-12])
    with pytest.raises(ValueError, match="IOError"):
        vc.convert(str(tmp_path / "cut.vcf.gz"), ref, outs[0])


def test_tid_and_region_filter_the_written_lines(ref, tmp_path):
    case = [c for c in GOLD["conversions"] if c["name"] == "plain"][0]
    src = write_case(tmp_path, case)[0]
    out = str(tmp_path / "out.txt")
    for tid, region in (("chr1", "60-205"), ("chr1", "61-206"), ("chr2", "0-1,000"), ("chrX", "0-1000")):
        a, b = [int(x.replace(",", "")) for x in region.split("-")]
        want = [l for l in case["lines"] if l.split(" ")[0] == tid and a <= int(l.split(" ")[1]) < b]
        assert vc.convert(src, ref, out, tid=tid, region=region) == len(want) and read(out) == "".join(l + "\n" for l in want)
        r = run_tool("dindel_vcf2candidates", ["-i", src, "-o", out, "-r", ref, "--tid", tid, "--region", region])
        assert r.returncode == 0 and read(out) == "".join(l + "\n" for l in want)
    assert [l for l in read(out)] == []                                                                       # (chrX: nothing)
    assert vc.convert(src, ref, out, tid="chr1", region="60-205") == 2


def test_python_module(ref, tmp_path):
    case = [c for c in GOLD["conversions"] if c["name"] == "two_files"][0]
    names = write_case(tmp_path, case)
    out = str(tmp_path / "out.txt")
    assert vc.convert(names, ref, out) == 4 and vc.convert(",".join(names), ref, out) == 4 and read(out).split("\n")[:-1] == case["lines"]
    assert vc.convert(names, ref, out, min_qual=51) == 0 and read(out) == ""
    assert vc.variant4("ACCCT", "AT") == ("del", 1, "-CCC") and vc.variant4("TC", "TTTC") == ("ins", 1, "+TT")
    with pytest.raises(ValueError, match="IOError.*none.vcf"):
        vc.convert(str(tmp_path / "none.vcf"), ref, out)
    with pytest.raises(ValueError, match="IOError.*none.fa"):
        vc.convert(names, str(tmp_path / "none.fa"), out)
    with pytest.raises(ValueError, match="go together"):
        vc.convert(names, ref, out, tid="chr1")


# ---------------------------------------------------------------- the tools' options
def test_tool_option_errors_and_help(ref, tmp_path):
    src = write_case(tmp_path, GOLD["conversions"][0])[0]
    out = str(tmp_path / "o.txt")
    for args, code, text in ((["-o", out, "-r", ref], 1, "Please specify --inputFile\n"), (["-i", src, "-r", ref], 1, "Please specify --outputFile\n"),
                             (["-i", src, "-o", out], 1, "Please specify --refFile\n"),
                             (["-i", src, "-o", out, "-r", ref, "--tid", "chr1"], 1, "--tid and --region go together: --tid NAME --region A-B\n"),
                             (["-i", src, "-o", out, "-r", ref, "--minQual", "high"], 1, "An error occurred!\nValueError: could not convert string to float: high\n"),
                             (["-i", src, "-o", out, "-r", ref, "--tid", "chr1", "--region", "x"], 1, "An error occurred!\nCannot parse region for start!\n"),
                             (["-i", src, "-o", out, "-r", ref, "--bogus"], 2, "dindel_vcf2candidates: error: no such option, or no value for it: --bogus\n"),
                             (["-i", src, "-o", out, "-r"], 2, "dindel_vcf2candidates: error: no such option, or no value for it: -r\n")):
        r = run_tool("dindel_vcf2candidates", args)
        assert (r.returncode, r.stderr) == (code, text), args
    r = run_tool("dindel_vcf2candidates", ["--inputFile", src, "--outputFile", out, "--refFile", ref, "--quiet"])
    assert r.returncode == 0 and r.stderr == "" and read(out).count("\n") == len(GOLD["conversions"][0]["lines"])
    warn = [c for c in GOLD["conversions"] if c["name"] == "no_info_lines_warns"][0]
    assert run_tool("dindel_vcf2candidates", ["-i", write_case(tmp_path, warn)[0], "-o", out, "-r", ref, "--quiet"]).stderr == ""
    h = run_tool("dindel_vcf2candidates", ["--help"])
    assert h.returncode == 0 and all(o in h.stdout for o in ("--inputFile", "--outputFile", "--refFile", "--minQual", "--tid", "--region", "--quiet"))


def test_dindel_gpu_option_errors_and_help(ref, tmp_path):
    base = ["--bamFile", "x.bam", "--outputFile", str(tmp_path / "err"), "--ref", ref]
    for args, text in ((base + ["--varFile", "w.txt", "--candidateVCF", "k.vcf"], "--candidateVCF adds known sites to the discovery stage: it needs --discover\n"),
                       (["--discover"] + base + ["--vcfCandidatesOnly"], "--vcfCandidatesOnly needs --candidateVCF\n"),
                       (["--discover"] + base + ["--candidateVCF", "k.vcf", "--vcfCandidatesOnly", "--useLibraries"],
                        "--useLibraries needs the pass over the BAM file: with --vcfCandidatesOnly the discovery stage writes no library file\n"),
                       (["--discover"] + base + ["--candidateVCF", "k.vcf", "--vcfCandidatesOnly", "--minCount", "2"],
                        "--minCount / --maxCount filter the sample's own candidates: with --vcfCandidatesOnly there are none\n"),
                       (["--discover"] + base + ["--candidateVCF", "k.vcf", "--vcfCandidatesOnly", "--maxCount", "9"],
                        "--minCount / --maxCount filter the sample's own candidates: with --vcfCandidatesOnly there are none\n"),
                       (["--discover"] + base + ["--candidateVCF", "k.vcf", "--minQual", "high"], "--minQual: ValueError: could not convert string to float: high\n")):
        r = run_tool("dindel_gpu", args)
        assert (r.returncode, r.stderr, r.stdout) == (1, text, ""), args
    r = run_tool("dindel_gpu", ["--discover"] + base + ["--candidateVCF"])
    assert r.returncode == 2 and r.stderr == "Option --candidateVCF needs a value\n"
    h = run_tool("dindel_gpu", ["--help"]).stdout
    assert all(o in h for o in ("--candidateVCF", "--minQual", "--vcfCandidatesOnly"))


# ---------------------------------------------------------------- the discovery stage with known sites
def in_library(symbol, name, args):
    lib = hostlib.load()
    fn = getattr(lib, symbol)
    fn.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
    argv = (C.c_char_p * (len(args) + 2))(name.encode(), *[str(a).encode() for a in args], None)
    return fn(len(args) + 1, argv)


def discover_vcf(prefix, fasta, vcf, bam=None, bam_list=None, tid=None, region=None, min_qual=1.0, vcf_only=False, min_dist=20, min_count=-1, max_count=-1,
                 batch_candidates=0, events_cap=0, host_convert=False, hook=cases.CHECKER_HOOK):
    lib = hostlib.load()
    lib.ddh_discover_windows_vcf.restype = C.c_long
    lib.ddh_discover_windows_vcf.argtypes = [C.c_char_p] * 7 + [C.c_double, C.c_int] + [C.c_long] * 3 + [C.c_int] * 3 + [cases.HOOK_TYPE, C.c_void_p, C.c_char_p, C.c_int]
    err = C.create_string_buffer(1024)
    enc = lambda s: None if s is None else str(s).encode()
    n = lib.ddh_discover_windows_vcf(enc(bam), enc(bam_list), enc(tid), enc(region), enc(fasta), enc(prefix), enc(vcf), min_qual, 1 if vcf_only else 0, min_dist,
                                     min_count, max_count, batch_candidates, events_cap, 1 if host_convert else 0, hook if hook is not None else cases.HOOK_TYPE(),
                                     None, err, len(err))
    if n < 0:
        raise RuntimeError(err.value.decode())
    return n


VCF_HEAD = '##fileformat=VCFv4.0\n##INFO=<ID=DP,Number=1,Type=Integer,Description="Total Depth">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n'


def vcf_del(name, seq, at, n, qual="50"):
    """the VCF record of the deletion of seq[at:at+n] (zero-based `at`)"""
    return "%s\t%d\t.\t%s\t%s\t%s\tPASS\tDP=1\n" % (name, at, seq[at - 1:at + n], seq[at - 1], qual)


def vcf_ins(name, seq, at, letters, qual="50"):
    """... of the insertion of `letters` in front of seq[at]"""
    return "%s\t%d\t.\t%s\t%s\t%s\tPASS\tDP=1\n" % (name, at, seq[at - 1], seq[at - 1] + letters, qual)


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    """the sample of tests/_discover_cases.py with a third target, chrC, in the FASTA that no read lies on; and a VCF naming a site the
    reads show too (chrA 900 +GAT), sites they do not show, a site inside chrA's homopolymer at a non-canonical base, chrC in two
    separate runs of records (the target comes back), and a record below --minQual"""
    tmp = tmp_path_factory.mktemp("vcfdiscover")
    s = dc.sample(tmp)
    import random
    rng = random.Random(77)
    chrC = "".join(rng.choice("ACGT") for _ in range(900))
    s["targets"]["chrC"] = chrC
    s["fasta"] = str(tmp / "three.fa")
    write_fasta(s["fasta"], [(n, s["targets"][n]) for n in ("chrA", "chrB", "chrC")])
    A, B = s["targets"]["chrA"], s["targets"]["chrB"]
    other = lambda c: "ACGT"[("ACGT".index(c) + 1) % 4]
    s["insB"], s["insC"] = "AC" + other(B[499]), other(chrC[699])          # leftmost as they stand: the base in front differs from the last inserted one
    assert A[1699] != A[1702]                                                # and so is the deletion at 1700
    s["vcf"] = str(tmp / "known.vcf")
    open(s["vcf"], "w").write(VCF_HEAD + vcf_del("chrC", chrC, 300, 2) + vcf_ins("chrA", A, 900, "GAT") + vcf_del("chrA", A, dc.RUN[0] + 4, 1) + vcf_del("chrA", A, 1700, 3) +
                              vcf_del("chrA", A, 1210, 1, qual="0.5") + vcf_ins("chrB", B, 500, s["insB"]) + vcf_del("chrC", chrC, 310, 1) + vcf_ins("chrC", chrC, 700, s["insC"]))
    s["vcf2"] = str(tmp / "more.vcf")
    open(s["vcf2"], "w").write(VCF_HEAD + vcf_del("chrB", B, 1404, 2) + vcf_del("chrA", A, 1130, 4))
    s["tmp"] = tmp
    return s


def chain(s, prefix, vcfs, bam_args, region=None, min_qual=None, vcf_only=False, window_filter=(), min_dist=()):
    """the tools inside the library, one after the other: every file of the stage under `prefix`"""
    region_args = ["--tid", region[0], "--region", region[1]] if region else []
    if not vcf_only:
        assert cases.run_in_library(["--analysis", "getCIGARindels", *bam_args, *region_args, "--ref", s["fasta"], "--outputFile",
                                     prefix + ".variants.txt" if region else prefix, "--quiet"]) == 0
    assert in_library("ddh_vcf2candidates_main", "dindel_vcf2candidates", ["-i", vcfs, "-o", prefix + ".vcf.variants.txt", "-r", s["fasta"], "--quiet", *region_args,
                                                                         *(["--minQual", min_qual] if min_qual is not None else [])]) == 0
    assert cases.run_in_library(["--analysis", "realignCandidates", "--varFile", prefix + ".vcf.variants.txt", "--ref", s["fasta"], "--outputFile",
                                 prefix + ".vcf.realigned", "--quiet"]) == 0
    kept = ""
    if not vcf_only:
        kept = read(prefix + ".variants.txt")
        if window_filter:
            assert in_library("ddh_windows_main", "dindel_windows", ["-i", prefix + ".variants.txt", "--oneFile", prefix + ".scratch", "--selectedFile", prefix + ".selected",
                                                                    "--quiet", *window_filter]) == 0
            kept = read(prefix + ".selected")
            os.remove(prefix + ".scratch"), os.remove(prefix + ".selected")
    open(prefix + ".candidates.txt", "w").write(kept + read(prefix + ".vcf.realigned.variants.txt"))
    assert in_library("ddh_windows_main", "dindel_windows", ["-i", prefix + ".candidates.txt", "--oneFile", prefix + ".windows.txt", "--quiet", *min_dist]) == 0


def files_of(prefix):
    d, base = os.path.split(prefix)
    return {f[len(base):]: read(os.path.join(d, f)) for f in os.listdir(d) if f.startswith(base + ".")}


BOTH = {".variants.txt", ".libraries.txt", ".vcf.variants.txt", ".vcf.realigned.variants.txt", ".candidates.txt", ".windows.txt"}
ONLY = {".vcf.variants.txt", ".vcf.realigned.variants.txt", ".candidates.txt", ".windows.txt"}


@pytest.fixture(scope="module")
def whole(sample):
    one, two = str(sample["tmp"] / "one"), str(sample["tmp"] / "two")
    n = discover_vcf(one, sample["fasta"], sample["vcf"], bam=sample["bam"])
    chain(sample, two, sample["vcf"], ["--bamFile", sample["bam"]])
    return one, two, n


def test_stage_files_equal_the_tools_in_a_row(whole):
    one, two, n = whole
    got, want = files_of(one), files_of(two)
    assert set(got) == BOTH and got == want and all(got.values())
    assert n == got[".windows.txt"].count("\n")


def test_both_sources_one_token_and_targets_in_order_of_appearance(sample, whole):
    one, _, _ = whole
    got = files_of(one)
    A, B, Cc = (sample["targets"][n] for n in ("chrA", "chrB", "chrC"))
    # what the script made of the records: file order, zero-based, the low-quality record gone
    assert got[".vcf.variants.txt"].split("\n")[:-1] == ["chrC 300 -" + Cc[300:302], "chrA 900 +GAT", "chrA %d -A" % (dc.RUN[0] + 4), "chrA 1700 -" + A[1700:1703],
                                                       "chrB 500 +" + sample["insB"], "chrC 310 -" + Cc[310], "chrC 700 +" + sample["insC"]]
    realigned = got[".vcf.realigned.variants.txt"].split("\n")[:-1]
    # the target that comes back gives two blocks; the deletion inside the homopolymer has moved to the run's canonical position, where the
    # sample's own candidate is; counts behind the realignment are the number of input lines, 1
    assert [l.split(" ")[0] for l in realigned] == ["chrC", "chrA", "chrA", "chrA", "chrB", "chrC", "chrC"] and all(l.endswith(" # 1") for l in realigned)
    own = [l for l in got[".variants.txt"].split("\n") if l.startswith("chrA ") and l.split(" ")[2] == "-A" and dc.RUN[0] - 2 <= int(l.split(" ")[1]) <= dc.RUN[1]]
    assert len(own) == 1
    run_pos = own[0].split(" ")[1]
    assert "chrA %s -A # 1" % run_pos in realigned and int(run_pos) != dc.RUN[0] + 4
    assert got[".candidates.txt"] == got[".variants.txt"] + got[".vcf.realigned.variants.txt"]
    lines = got[".windows.txt"].split("\n")[:-1]
    assert [k for k, _ in __import__("itertools").groupby(l.split(" ")[0] for l in lines)] == ["chrA", "chrB", "chrC"]      # the VCF's own target follows the BAM's
    tokens = [t for l in lines for t in l.split(" ")[3:]]
    assert tokens.count("900,+GAT") == 1 and tokens.count("%s,-A" % run_pos) == 1                         # named by both sources: one token
    assert "1700,-" + A[1700:1703] in tokens and "500,+" + sample["insB"] in tokens and "700,+" + sample["insC"] in tokens
    assert [l for l in lines if "300,-" in l][0].split(" ")[3:] == ["300,-" + Cc[300:302], "310,-" + Cc[310]]   # chrC's two blocks are one target again
    assert len(lines) == 8 + 4


@pytest.mark.parametrize("name,kw,chain_kw", [
    ("minCount2", dict(min_count=2), dict(window_filter=("--minCount", "2"))),
    ("maxCount12minDist25", dict(max_count=12, min_dist=25, batch_candidates=3, host_convert=True), dict(window_filter=("--maxCount", "12"), min_dist=("-m", "25"))),
    ("minQual", dict(min_qual=0.5, events_cap=1), dict(min_qual="0.5")),
    ("only", dict(vcf_only=True), dict(vcf_only=True)),
    ("twoFiles", dict(two=True), dict()),
], ids=lambda x: x if isinstance(x, str) else "")
def test_stage_with_options_equals_the_tools_with_the_same_options(sample, whole, name, kw, chain_kw):
    kw = dict(kw)
    vcfs = sample["vcf"] + "," + sample["vcf2"] if kw.pop("two", False) else sample["vcf"]
    a, b = str(sample["tmp"] / (name + "_a")), str(sample["tmp"] / (name + "_b"))
    only = kw.get("vcf_only", False)
    discover_vcf(a, sample["fasta"], vcfs, bam=None if only else sample["bam"], **kw)
    chain(sample, b, vcfs, ["--bamFile", sample["bam"]], **chain_kw)
    got, want = files_of(a), files_of(b)
    assert set(got) == (ONLY if only else BOTH) and got == want
    plain = files_of(whole[0])
    if name == "minCount2":                            # the filter acts on the sample's candidates only: every known site stays, count 1 and all
        assert got[".candidates.txt"].endswith(got[".vcf.realigned.variants.txt"]) and got[".vcf.realigned.variants.txt"] == plain[".vcf.realigned.variants.txt"]
        assert " +TT #" not in got[".candidates.txt"] and " +TT #" in plain[".candidates.txt"] and "700,+" + sample["insC"] in got[".windows.txt"]
    if name == "minQual":
        assert " 1210 -" in got[".vcf.variants.txt"] and " 1210 -" not in plain[".vcf.variants.txt"]
    if name == "only":
        assert got[".candidates.txt"] == got[".vcf.realigned.variants.txt"] == plain[".vcf.realigned.variants.txt"]
        assert [k for k, _ in __import__("itertools").groupby(l.split(" ")[0] for l in got[".windows.txt"].split("\n")[:-1])] == ["chrC", "chrA", "chrB"]
    if name == "twoFiles":
        assert got[".vcf.variants.txt"].startswith(plain[".vcf.variants.txt"]) and got[".vcf.variants.txt"].count("\n") == 9


def test_region_run_over_two_files_equals_the_tools(sample):
    a, b = str(sample["tmp"] / "region_a"), str(sample["tmp"] / "region_b")
    discover_vcf(a, sample["fasta"], sample["vcf"], bam_list=sample["list"], tid="chrA", region="850-1,750")
    chain(sample, b, sample["vcf"], ["--bamFiles", sample["list"]], region=("chrA", "850-1,750"))
    got, want = files_of(a), files_of(b)
    assert set(got) == BOTH - {".libraries.txt"} and got == want
    assert [l.split(" ")[1] for l in got[".vcf.variants.txt"].split("\n")[:-1]] == ["900", "1700"]


def test_run_without_candidate_vcf_writes_what_it_wrote_before(sample, tmp_path):
    """no --candidateVCF: the entry with known sites and the entry from before it write the same three files, and no others"""
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    na = discover_vcf(a, sample["fasta"], None, bam=sample["bam"], min_count=2)
    nb = dc.discover_in_library(b, sample["fasta"], bam=sample["bam"], min_count=2)
    assert na == nb and files_of(a) == files_of(b) and set(files_of(a)) == {".variants.txt", ".libraries.txt", ".windows.txt"}
    assert cases.run_in_library(["--analysis", "getCIGARindels", "--bamFile", sample["bam"], "--ref", sample["fasta"], "--outputFile", b + "c", "--quiet"]) == 0
    assert in_library("ddh_windows_main", "dindel_windows", ["-i", b + "c.variants.txt", "--oneFile", b + "c.windows.txt", "--minCount", "2", "--quiet"]) == 0
    assert files_of(b + "c") == files_of(a)


def test_stage_errors(sample, tmp_path):
    x = str(tmp_path / "x")
    with pytest.raises(RuntimeError, match="--vcfCandidatesOnly needs --candidateVCF"):
        discover_vcf(x, sample["fasta"], None, bam=sample["bam"], vcf_only=True)
    with pytest.raises(RuntimeError, match="with --vcfCandidatesOnly there are none"):
        discover_vcf(x, sample["fasta"], sample["vcf"], vcf_only=True, min_count=2)
    with pytest.raises(RuntimeError, match="No BAM file to discover candidates in"):
        discover_vcf(x, sample["fasta"], sample["vcf"])
    bad = str(tmp_path / "bad.vcf")
    open(bad, "w").write(VCF_HEAD + "chrA\t100\t.\tA\tTA\t50\tPASS\tDP=1\n")
    with pytest.raises(RuntimeError, match="Don't think this is a proper VCF4 insertion"):         # a conversion that fails stops the stage: no window file
        discover_vcf(x, sample["fasta"], bad, vcf_only=True)
    assert not os.path.exists(x + ".windows.txt") and not os.path.exists(x + ".candidates.txt")
    with pytest.raises(RuntimeError, match="IOError"):
        discover_vcf(x, sample["fasta"], str(tmp_path / "none.vcf"), bam=sample["bam"])
    assert not os.path.exists(x + ".windows.txt")


# ---------------------------------------------------------------- citations
def test_citations_of_the_new_files_point_inside_the_reference():
    nlines = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_line_counts.json")))["nlines"]
    pat = re.compile(r"((?:python/)?[A-Za-z][A-Za-z0-9_]*\.(?:cpp|hpp|py|h))`?:(\d+)(?:-(\d+))?")
    bad, n = [], 0
    for rel in ("dindel_tgi_amd/host/vcf_candidates.hpp", "dindel_tgi_amd/host/vcf_candidates.cpp", "dindel_tgi_amd/host/vcf_candidates_main.cpp",
                "dindel_tgi_amd/host/discover.hpp", "tests/golden/make_vcf_candidates_fixtures.py"):
        for m in pat.finditer(read(os.path.join(ROOT, rel))):
            name, a, b = m.group(1), int(m.group(2)), int(m.group(3) or m.group(2))
            if name not in nlines:
                continue
            n += 1
            if not (1 <= a <= b <= nlines[name]):
                bad.append((rel, m.group(0), nlines[name]))
    assert {"VCFFile.py", "Variant.py", "Fasta.py", "python/convertVCFToDindel.py"} <= set(nlines)
    assert n > 30 and not bad, (n, bad)


def test_fixture_file_holds_no_script_text():
    text = read(os.path.join(ROOT, "tests", "golden", "vcf_candidates.json"))
    assert set(GOLD) == {"variant4", "conversions", "fasta", "fai"}
    for word in ("def ", "import ", "self.", "class ", "lambda"):
        assert word not in text, word
