"""The end of the pooled workflow (host/pooled_vcf.cpp, dindel_pooled2vcf, dindel_pooled2glf, dindel_tgi_amd/pooled_vcf.py, the pooled
analysis' choice of the haplotype a read is realigned to) without a GPU.

What the two conversions write is pinned against tests/golden/pooled_vcf.json, which tests/golden/make_pooled_vcf_fixtures.py recorded from
the reference's own python/mergeOutputPooled.py and python/makeGenotypeLikelihoodFilePooled.py: VCF and likelihood file byte for byte — the
lines of one (chromosome, position) as a sorted list, the one order that is a Python-2 hash table's in the script —, stderr and stdout
exactly, a NameError's text exactly, any other exception of the scripts by the fact that the conversion dies and by its type."""
import ctypes as C
import gzip
import json
import os
import re
import subprocess

import pytest

from dindel_tgi_amd import hostlib, pooled_vcf as pv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dindel_tgi_amd", "host")
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "pooled_vcf.json")))
# Python 2 names -> what Python 3, which recorded the fixtures, calls the same exception
PY3_TYPE = {"IOError": "OSError"}


def unpack(ids):
    """a text of the fixture: indices into GOLD["lines"], where a row of the .glf.txt table is kept as [column, cell, ...] against the default row"""
    out = []
    for e in (GOLD["lines"][i] for i in ids):
        if not isinstance(e, str):
            cells = list(GOLD["default_row"])
            for col, cell in zip(e[0::2], e[1::2]):
                cells[col] = cell
            e = " ".join(cells) + "\n"
        out.append(e)
    return "".join(out)


for _c in GOLD["merges"] + GOLD["glfs"]:
    for _f in _c["files"]:
        _f["text"] = None if _f["text"] is None else unpack(_f["text"])
    for _k in ("vcf", "output", "stderr", "stdout"):
        if _k in _c:
            _c[_k] = unpack(_c[_k])
MERGES = {c["name"]: c for c in GOLD["merges"]}
GLFS = {c["name"]: c for c in GOLD["glfs"]}


@pytest.fixture(scope="module", autouse=True)
def built():
    hostlib.load()
    if not all(os.path.exists(os.path.join(HOST, t)) for t in ("dindel_pooled2vcf", "dindel_pooled2glf", "dindel_gpu")):
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
    with open(path, mode, **({} if "b" in mode else {"newline": ""})) as f:
        return f.read()


def put(path, text):
    with open(path, "w", newline="") as f:
        f.write(text)


def died_as(thrown, error):
    """the thrown text against the recorded exception: a NameError's text exactly, any other by its type"""
    if error["type"] == "NameError":
        return thrown == error["text"]
    kind = thrown.split(":")[0]
    return PY3_TYPE.get(kind, kind) == error["type"]


def by_site(vcf):
    """the VCF's lines with the lines of one (chromosome, position) sorted: runs of data lines with the same two first fields"""
    out, run, key = [], [], None
    for line in vcf.split("\n"):
        k = tuple(line.split("\t")[:2]) if line and not line.startswith("#") else None
        if k != key or k is None:
            out += sorted(run)
            run, key = [], k
        run.append(line)
    return out + sorted(run)


def write_files(tmp, case):
    paths = [str(tmp / f["name"]) for f in case["files"]]
    for f, p in zip(case["files"], paths):
        if f["text"] is not None:
            put(p, f["text"])
    put(str(tmp / "list.txt"), "".join(l.format(*paths) + "\n" for l in case["list"]))
    return str(tmp / "list.txt")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    d = tmp_path_factory.mktemp("pooledref")
    put(str(d / "ref.fa"), GOLD["fasta"])
    put(str(d / "ref.fa.fai"), GOLD["fai"])
    return str(d / "ref.fa")


def there(text, tmp, ref):
    """a recorded text with this run's directory; the reference FASTA lies elsewhere"""
    return text.replace("{DIR}/ref.fa", ref).replace("{DIR}", str(tmp))


# ---------------------------------------------------------------- mergeOutputPooled.py
@pytest.mark.parametrize("case", GOLD["merges"], ids=lambda c: c["name"])
def test_merge_in_the_library_and_by_the_tool(case, ref, tmp_path):
    lst = write_files(tmp_path, case)
    o = case["options"]
    out_l, out_t = str(tmp_path / "lib.vcf"), str(tmp_path / "tool.vcf")
    got = pv.merge_with_notes(lst, ref, out_l, o["numSamples"], o["numBamFiles"], o["maxHPLen"], o["filterFR"], o["filterQual"])
    r = run_tool("dindel_pooled2vcf", ["-i", lst, "-o", out_t, "-r", ref, "--numSamples", o["numSamples"], "--numBamFiles", o["numBamFiles"], "--maxHPLen", o["maxHPLen"],
                                       "--filterQual", o["filterQual"]] + (["--filterFR"] if o["filterFR"] else []))
    assert got["stderr"] == there(case["stderr"], tmp_path, ref) == r.stderr[:len(got["stderr"])]
    want_stdout = there(case["stdout"], tmp_path, ref)
    if case["name"] == "chromosome_names_outside_the_list":      # the progress lines per chromosome follow the order of the chromosomes: the recorder's is a Python-3 set's there
        assert sorted(got["stdout"].split("\n")) == sorted(want_stdout.split("\n")) and r.stdout == got["stdout"]
    else:
        assert got["stdout"] == want_stdout == r.stdout
    if "error" in case:
        assert "throw" in got and died_as(got["throw"], case["error"]), (got, case["error"])
        assert r.returncode == 1 and r.stderr == got["stderr"] + "An error occurred!\n" + got["throw"] + "\n"
        with pytest.raises(ValueError) as e:
            pv.merge(lst, ref, out_l, o["numSamples"], o["numBamFiles"], o["maxHPLen"], o["filterFR"], o["filterQual"])
        assert str(e.value) == got["throw"]
    else:
        assert "throw" not in got, got
        want = there(case["output"], tmp_path, ref)
        assert by_site(read(out_l)) == by_site(want)
        assert read(out_l).split("#CHROM")[0] == want.split("#CHROM")[0]
        assert r.returncode == 0 and read(out_t) == read(out_l) and r.stderr == got["stderr"]


def test_merge_fixture_holds_the_cases_the_rules_need():
    def data(name):
        return [l.split("\t") for l in MERGES[name]["output"].split("\n") if l and not l.startswith("#")]

    assert [l[6] for l in data("two_sites_5bp_apart_both_stay_pass")] == ["PASS", "PASS"] and [l[1] for l in data("two_sites_5bp_apart_both_stay_pass")] == ["100", "105"]
    assert [l[6] for l in data("filtered_beside_pass_gets_tc10")][:3] == ["PASS", "PASS", "q20;tc10"]           # 155: the PASS variant stays PASS, the filtered one gets tc10
    tie = [(int(l[1]), l[6]) for l in data("tie_in_qual_across_positions")]
    assert tie == [(300, "PASS"), (300, "q20"), (306, "PASS"), (306, "q20;tc10"), (312, "PASS"), (312, "q20;tc10")]   # the lowest position is the best one
    assert data("one_depth_value_only") == [] and "coverage range 34 0\"" in MERGES["one_depth_value_only"]["output"]
    assert {l[0] for l in data("chromosome_with_only_filtered_variants")} == {"1"}                               # chromosome 2: no line at all
    assert [l[0] for l in data("chromosome_names_outside_the_list")] == ["1", "2", "10", "X", "GL000207.1", "chrA", "chrA", "chrB"]
    assert [l[6] for l in data("numSamples_3_with_NS_1_is_not_s50")] == ["PASS", "s50", "PASS"] and "NS=1;" in data("numSamples_3_with_NS_1_is_not_s50")[0][7]
    assert [l[6] for l in data("numSamples_4_with_NS_1_is_s50")] == ["s50", "s50", "PASS"]
    assert [l[6] for l in data("filterFR")] == ["fr0", "fr0", "PASS"] and "ID=fr0" in MERGES["filterFR"]["output"] and "fr0" not in MERGES["without_filterFR"]["output"]
    assert [l[5] for l in data("post_prob_variant_0.999_is_qual_29")] == ["29", "19", "99", "100", "100", "20"]
    assert [l[1] for l in data("interleaved_dip_lines_NA_lines_short_last_group")] == ["100", "200", "300"]
    assert MERGES["wrong_field_count"]["error"]["type"] == "TypeError" and "correct number of labels" in MERGES["wrong_field_count"]["stderr"]
    assert MERGES["snp_line_above_0.2"]["error"] == dict(type="IndexError", text="string index out of range")
    texts = {c["error"]["text"] for c in GOLD["merges"] if "error" in c and c["error"]["type"] == "NameError"}
    assert texts == {"Error. Is the number of BAM files correctly specified?", "Inconsistent glf files! Is the number of BAM files correctly specified?",
                     "GLF files are corrupt. Could not find all required columns.", "KeyError", "Unrecognized variant: ACGT"}
    info = data("how_AF_is_written")
    assert [l[7].split(";")[0] for l in info] == ["AF=1.0", "AF=0.5", "AF=0.123456789012", "AF=1e-05", "AF=0.0001", "AF=0.25", "AF=1.5", "AF=100.0"]


def test_gz_gives_the_bytes_of_the_plain_file(ref, tmp_path):
    case = MERGES["filtered_beside_pass_gets_tc10"]
    lst = write_files(tmp_path, case)
    plain = str(tmp_path / case["files"][0]["name"])
    text = read(plain, "rb")
    one, members = str(tmp_path / "one.glf.txt.gz"), str(tmp_path / "members.glf.txt.gz")
    with gzip.open(one, "wb") as f:
        f.write(text)
    cut = [0, 40, 41, len(text) // 2, len(text)]
    with open(members, "wb") as f:                     # one gzip member per piece, as bgzip writes one per block, and its empty last member
        for a, b in zip(cut, cut[1:]):
            f.write(gzip.compress(text[a:b]))
        f.write(gzip.compress(b""))
    outs = []
    for k, src in enumerate((plain, one, members)):
        put(lst, src + "\n")
        outs.append(str(tmp_path / ("out%d.vcf" % k)))
        pv.merge(lst, ref, outs[-1], 2, 2)
    assert read(outs[0]) == read(outs[1]) == read(outs[2]) and by_site(read(outs[0])) == by_site(there(case["output"], tmp_path, ref))
    glf = GLFS["q20_with_qual_9_and_10"]
    put(str(tmp_path / "calls.vcf"), glf["vcf"])
    put(str(tmp_path / "g.glf.txt"), glf["files"][0]["text"])
    with gzip.open(str(tmp_path / "g.glf.txt.gz"), "wb") as f:
        f.write(glf["files"][0]["text"].encode())
    put(str(tmp_path / "bams.txt"), "".join(b + "\n" for b in glf["bams"]))
    for k, src in enumerate(("g.glf.txt", "g.glf.txt.gz")):
        put(lst, str(tmp_path / src) + "\n")
        pv.make_glf(lst, str(tmp_path / "calls.vcf"), str(tmp_path / ("glf%d.txt" % k)), str(tmp_path / "bams.txt"))
    assert read(str(tmp_path / "glf0.txt")) == read(str(tmp_path / "glf1.txt")) == glf["output"]
    with open(str(tmp_path / "cut.glf.txt.gz"), "wb") as f:
        f.write(read(one, "rb")[:-12])
    put(lst, str(tmp_path / "cut.glf.txt.gz") + "\n")
    with pytest.raises(ValueError, match="IOError"):
        pv.merge(lst, ref, outs[0], 2, 2)


def test_percentiles_table_from_the_script():
    assert len(GOLD["percentiles"]) >= 10
    for hist, pct, want in GOLD["percentiles"]:
        assert pv.percentiles({int(k): v for k, v in hist}, pct) == want, (hist, pct)
    assert pv.percentiles({20: 5}) == [20, 0]                                            # one depth value: at most one percentile advances per depth


# ---------------------------------------------------------------- makeGenotypeLikelihoodFilePooled.py
@pytest.mark.parametrize("case", GOLD["glfs"], ids=lambda c: c["name"])
def test_make_glf_in_the_library_and_by_the_tool(case, ref, tmp_path):
    lst = write_files(tmp_path, case)
    calls, bams = str(tmp_path / case["vcf_name"]), str(tmp_path / "bams.txt")
    put(calls, case["vcf"])
    put(bams, "".join(b + "\n" for b in case["bams"]))
    out_l, out_t = str(tmp_path / "lib.txt"), str(tmp_path / "tool.txt")
    got = pv.make_glf_with_notes(lst, calls, out_l, bams)
    r = run_tool("dindel_pooled2glf", ["-g", lst, "-c", calls, "-o", out_t, "-b", bams])
    assert got["stderr"] == there(case["stderr"], tmp_path, ref) and got["stdout"] == there(case["stdout"], tmp_path, ref) == r.stdout
    if "error" in case:
        assert "throw" in got and died_as(got["throw"], case["error"]), (got, case["error"])
        assert r.returncode == 1 and r.stderr == got["stderr"] + got["throw"] + "\n"
        with pytest.raises(ValueError) as e:
            pv.make_glf(lst, calls, out_l, bams)
        assert str(e.value) == got["throw"]
    else:
        assert "throw" not in got, got
        assert read(out_l) == case["output"]
        assert r.returncode == 0 and read(out_t) == read(out_l) and r.stderr == got["stderr"]


def test_glf_fixture_holds_the_cases_the_rules_need():
    kept = [l.split(" ")[:3] for l in GLFS["q20_with_qual_9_and_10"]["output"].split("\n")[:-1:2]]
    assert kept == [["1", "100", "-AC"], ["1", "250", "-T"], ["2", "50", "+TT"]]          # PASS; q20 with 10 and 10.5; not q20 with 9, q20;tc10, hp10
    assert GLFS["group_of_the_wrong_length"]["stderr"] == "Skipping index 1.100.-AC\nSkipping index 3.250.-T\n"
    assert GLFS["dip_map_line_of_a_called_site"]["error"]["type"] == "KeyError"
    assert GLFS["two_files_with_the_same_first_position"]["error"] == dict(type="NameError", text="Huh?")
    assert [l.split(" ")[:2] for l in GLFS["files_in_the_order_of_their_first_position"]["output"].split("\n")[:-1:2]] == [["2", "50"], ["1", "250"], ["1", "100"]]
    texts = {c["error"]["text"] for c in GOLD["glfs"] if "error" in c and c["error"]["type"] == "NameError"}
    assert texts == {"Cannot deal with these entries", "Multiple same variants?", "Huh?", "MultiSNP", "Don't think this is a proper VCF4 insertion"}


def test_variant4_of_equal_lengths_from_the_script():
    assert len(GOLD["variant4"]) > 80
    for r, a, typ, off, s in GOLD["variant4"]:
        try:
            got = pv.variant4(r, a)
        except ValueError as e:
            assert typ is None and died_as(str(e), dict(type=s[0], text=s[1])), (r, a, str(e), s)
        else:
            assert got == (typ, off, s), (r, a)
    assert pv.variant4("GAC", "GAT") == ("snp", 2, "C=>T") and pv.variant4("ACCCT", "AT") == ("del", 1, "-CCC")      # unequal lengths: variant4 as it was


def test_python_module(ref, tmp_path):
    case = MERGES["two_sites_5bp_apart_both_stay_pass"]
    lst = write_files(tmp_path, case)
    out = str(tmp_path / "o.vcf")
    assert pv.merge(lst, ref, out, num_samples=2, num_bam_files=2) is None
    assert [l.split("\t")[6] for l in read(out).split("\n") if l and l[0] != "#"] == ["PASS", "PASS"]
    pv.merge(lst, ref, out, num_samples=2, num_bam_files=2, filter_qual=40)
    assert [l.split("\t")[6] for l in read(out).split("\n") if l and l[0] != "#"] == ["PASS", "q40"]
    with pytest.raises(ValueError, match="IOError.*none.fa"):
        pv.merge(lst, str(tmp_path / "none.fa"), out, 2, 2)
    with pytest.raises(ValueError, match="IOError.*nolist.txt"):
        pv.merge(str(tmp_path / "nolist.txt"), ref, out, 2, 2)
    with pytest.raises(ValueError, match="IOError.*none.vcf"):
        pv.make_glf(lst, str(tmp_path / "none.vcf"), out, lst)


def test_notes_larger_than_the_buffer_and_bytes_outside_ascii(ref, tmp_path):
    """a result beyond the first buffer is fetched, not computed again (the output file is written once); a path that is not ASCII reaches
    Python as it is"""
    d = tmp_path / "pöols"
    d.mkdir()
    glf = str(d / "mänge.glf.txt")
    put(glf, MERGES["two_sites_5bp_apart_both_stay_pass"]["files"][0]["text"])
    lst, out = str(tmp_path / "many.txt"), str(tmp_path / "o.vcf")
    put(lst, (str(d / "gone.glf.txt") + "\n") * 700 + glf + "\n")
    got = pv.merge_with_notes(lst, ref, out, 2, 2)
    assert got["stderr"] == ("WARNING: GLF file %s does not exist.\n" % str(d / "gone.glf.txt")) * 700 and len(got["stderr"].encode()) > (1 << 16)
    assert got["stdout"].startswith("Reading %s\n" % glf) and read(out).count("\tPASS\t") == 2
    with pytest.raises(ValueError) as e:
        pv.merge(lst, str(d / "nö.fa"), out, 2, 2)
    assert str(d / "nö.fa") in str(e.value)


# ---------------------------------------------------------------- the tools' options
def test_tool_option_errors_and_help(ref, tmp_path):
    lst = write_files(tmp_path, MERGES["two_sites_5bp_apart_both_stay_pass"])
    out = str(tmp_path / "o.vcf")
    full = ["-i", lst, "-o", out, "-r", ref, "--numSamples", "2", "--numBamFiles", "2"]
    for args, code, text in ((["-o", out, "-r", ref, "--numSamples", "2"], 1, "Please specify --inputFiles\n"), (["-i", lst, "-r", ref, "--numSamples", "2"], 1, "Please specify --outputFile\n"),
                             (["-i", lst, "-o", out, "--numSamples", "2"], 1, "Please specify --refFile\n"), (["-i", lst, "-o", out, "-r", ref], 1, "Please specify --numSamples option\n"),
                             (full + ["--filterQual", "high"], 1, "An error occurred!\nValueError: invalid literal for int() with base 10: 'high'\n"),
                             (full + ["--maxHPLen", "x"], 2, "dindel_pooled2vcf: error: option --maxHPLen: invalid integer value: 'x'\n"),
                             (full + ["--bogus"], 2, "dindel_pooled2vcf: error: no such option, or no value for it: --bogus\n"),
                             (["-i", lst, "-o", out, "-r"], 2, "dindel_pooled2vcf: error: no such option, or no value for it: -r\n")):
        r = run_tool("dindel_pooled2vcf", args)
        assert (r.returncode, r.stderr) == (code, text), args
    r = run_tool("dindel_pooled2vcf", ["--inputFiles", lst, "--outputFile", out, "--refFile", ref, "--numSamples", "2", "--numBamFiles", "2", "--quiet"])
    assert (r.returncode, r.stdout, r.stderr) == (0, "", "") and read(out).count("\tPASS\t") == 2
    h = run_tool("dindel_pooled2vcf", ["--help"])
    assert h.returncode == 0 and all(o in h.stdout for o in ("--inputFiles", "--outputFile", "--refFile", "--numSamples", "--numBamFiles", "--maxHPLen", "--filterFR", "--filterQual"))
    for args in (["-c", out, "-o", out, "-b", lst], ["-g", lst, "-o", out, "-b", lst], ["-g", lst, "-c", out, "-b", lst], ["-g", lst, "-c", out, "-o", out], []):
        r = run_tool("dindel_pooled2glf", args)
        assert (r.returncode, r.stderr) == (1, "Please specify all required options.\n"), args
    r = run_tool("dindel_pooled2glf", ["-g", lst, "-c", out, "-o", out + ".glf", "-b", lst, "--bogus"])
    assert (r.returncode, r.stderr) == (2, "dindel_pooled2glf: error: no such option, or no value for it: --bogus\n")
    put(str(tmp_path / "bams.txt"), "a.bam\nb.bam\n")
    r = run_tool("dindel_pooled2glf", ["--inputGLFFiles", lst, "--callFile", out, "--outputFile", out + ".glf", "--bamFiles", str(tmp_path / "bams.txt"), "--quiet"])
    assert (r.returncode, r.stdout, r.stderr) == (0, "", "") and read(out + ".glf") == "1 105 +G -10.5 -2.25 -30 a.bam\n1 105 +G -11.5 -2.25 -31 b.bam\n"
    h = run_tool("dindel_pooled2glf", ["--help"])
    assert h.returncode == 0 and all(o in h.stdout for o in ("--inputGLFFiles", "--callFile", "--outputFile", "--bamFiles"))


def test_dindel_gpu_option_errors_and_help(ref, tmp_path):
    base = ["--bamFile", "x.bam", "--varFile", "w.txt", "--outputFile", str(tmp_path / "err")]
    for args, text in ((base + ["--ref", ref, "--pooledVcf", "p.vcf", "--numSamples", "3"], "--pooledVcf converts the lines of the pooled analysis: it needs --doPooled\n"),
                       (base + ["--hapFile", "h.txt", "--doPooled", "--pooledVcf", "p.vcf", "--numSamples", "3"], "Please specify --ref: --pooledVcf needs the reference FASTA\n"),
                       (base + ["--ref", ref, "--doPooled", "--pooledVcf", "p.vcf"], "Please specify --numSamples: --pooledVcf needs the number of samples in the pools\n"),
                       (base + ["--ref", ref, "--doPooled", "--pooledGlf", "p.glf", "--numSamples", "3"], "--pooledGlf writes the likelihoods of the sites --pooledVcf calls: it needs --pooledVcf\n"),
                       (base + ["--ref", ref, "--doPooled", "--pooledVcf", "p.vcf", "--numSamples", "three"], "--numSamples: ValueError: invalid literal for int() with base 10: 'three'\n")):
        r = run_tool("dindel_gpu", args)
        assert (r.returncode, r.stderr, r.stdout) == (1, text, ""), args
    r = run_tool("dindel_gpu", base + ["--ref", ref, "--doPooled", "--pooledVcf"])
    assert r.returncode == 2 and r.stderr == "Option --pooledVcf needs a value\n"
    # --doPooled --outputRealignedBAM without --doDiploid is not refused: a note says whose files they are, and the run gets as far as its BAM file
    r = run_tool("dindel_gpu", base + ["--ref", ref, "--doPooled", "--outputRealignedBAM"])
    assert r.returncode == 1 and r.stderr.startswith("--doPooled --outputRealignedBAM without --doDiploid: the files are the pooled analysis' own")
    assert r.stderr.endswith("Exception: Cannot open BAM file.\n") and "needs --doDiploid" not in r.stderr
    assert run_tool("dindel_gpu", base + ["--ref", ref, "--doPooled", "--outputRealignedBAM", "--quiet"]).stderr == "Exception: Cannot open BAM file.\n"
    h = run_tool("dindel_gpu", ["--help"]).stdout
    assert all(o in h for o in ("--pooledVcf", "--pooledGlf", "--numSamples"))


# ---------------------------------------------------------------- the pooled analysis' realigned reads
def test_pooled_realigned_cigars_take_the_first_maximum():
    lib = hostlib.load()
    lib.ddh_pooled_realigned_cigars.argtypes = [C.POINTER(C.c_double), C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    inf, nan = float("inf"), float("nan")
    #        read:  0      1      2      3      4      5      6
    ll = [[-5.0, -1.0, -inf, -3.0, -2.0, nan, -7.0],      # haplotype 0
          [-2.0, -1.0, -inf, -3.0, -2.0, nan, -7.0],      # haplotype 1
          [-2.0, -4.0, -inf, -1.0, -2.0, -9.0, -6.5],     # haplotype 2
          [-9.0, -1.0, -inf, -1.0, -1.5, nan, -6.5]]      # haplotype 3
    on_hap = [1, 1, 1, 1, 0, 1, 1]
    H, R = len(ll), len(on_hap)
    flat = (C.c_double * (H * R))(*[x for row in ll for x in row])
    nops, ref_pos = (C.c_int * R)(), (C.c_int * R)()
    assert lib.ddh_pooled_realigned_cigars(flat, H, R, (C.c_int * R)(*on_hap), 36, 1000, nops, ref_pos) == 0
    # read 0: haplotypes 1 and 2 tie, the first wins; 1: 0, 1 and 3 tie; 2: all -inf, nothing compares greater: haplotype 0; 3: 2 and 3 tie;
    # 4: not on a haplotype: an empty CIGAR; 5: NaN never compares greater: haplotype 2; 6: 2 and 3 tie
    assert list(ref_pos) == [1010, 1000, 1000, 1020, -1, 1020, 1020]
    assert list(nops) == [1, 1, 1, 1, 0, 1, 1]


# ---------------------------------------------------------------- the stand-alone program under the sanitizers
def test_check_program_under_address_and_undefined_sanitizers(tmp_path):
    """tests/pooled_vcf_check.cpp with host/pooled_vcf.cpp and the two units it stands on, g++ alone, under AddressSanitizer and UBSan; run directly."""
    exe = str(tmp_path / "pooled_vcf_check")
    subprocess.check_call(["g++", "-std=c++11", "-O0", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "pooled_vcf_check.cpp"), os.path.join(HOST, "pooled_vcf.cpp"), os.path.join(HOST, "vcf_candidates.cpp"),
                           os.path.join(HOST, "glf_to_vcf.cpp"), "-lz"])
    work = tmp_path / "work"
    work.mkdir()
    r = subprocess.run([exe, str(work)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.endswith("ok\n") and r.stderr == "", (r.stdout[-2000:], r.stderr[-4000:])


# ---------------------------------------------------------------- citations
def test_citations_of_the_new_files_point_inside_the_reference():
    nlines = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_line_counts.json")))["nlines"]
    pat = re.compile(r"((?:python/)?[A-Za-z][A-Za-z0-9_]*\.(?:cpp|hpp|py|h))`?:(\d+)(?:-(\d+))?")
    bad, n = [], 0
    for rel in ("dindel_tgi_amd/host/pooled_vcf.hpp", "dindel_tgi_amd/host/pooled_vcf.cpp", "dindel_tgi_amd/host/pooled_vcf_main.cpp", "dindel_tgi_amd/host/realigned_bam.hpp",
                "dindel_tgi_amd/host/realigned_bam.cpp", "tests/golden/make_pooled_vcf_fixtures.py"):
        for m in pat.finditer(read(os.path.join(ROOT, rel))):
            name, a, b = m.group(1), int(m.group(2)), int(m.group(3) or m.group(2))
            if name not in nlines:
                continue
            n += 1
            if not (1 <= a <= b <= nlines[name]):
                bad.append((rel, m.group(0), nlines[name]))
    assert {"FileUtils.py", "Variant.py", "python/mergeOutputPooled.py", "python/makeGenotypeLikelihoodFilePooled.py"} <= set(nlines)
    assert n > 30 and not bad, (n, bad)


def test_fixture_file_holds_no_script_text():
    text = read(os.path.join(ROOT, "tests", "golden", "pooled_vcf.json"))
    assert set(GOLD) == {"variant4", "percentiles", "merges", "glfs", "fasta", "fai", "lines", "default_row"}
    for word in ("def ", "import ", "self.", "class ", "lambda"):
        assert word not in text, word
