"""The discovery stage of dindel_gpu --discover (host/discover.cpp) without a GPU: ddh_discover_windows with the checker's alignments
injected through the library's hook, as tests/test_candidates_cpu.py runs the candidate tool.  Its three by-products must be the bytes
of the two tools run one after the other (ddh_candidates_main, then ddh_windows_main), and the sample's implanted indels must come out
as the windows they were planted to make."""
import ctypes as C

import pytest

from dindel_tgi_amd import hostlib
from tests import _candidates_cases as cases, _discover_cases as dc


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    return dc.sample(tmp_path_factory.mktemp("discover"))


def windows_in_library(args):
    lib = hostlib.load()
    lib.ddh_windows_main.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
    argv = (C.c_char_p * (len(args) + 2))(b"dindel_windows", *[str(a).encode() for a in args], None)
    return lib.ddh_windows_main(len(args) + 1, argv)


def read(path):
    return open(path).read()


@pytest.fixture(scope="module")
def whole(sample, tmp_path_factory):
    """the stage and the chain on the whole file, once"""
    tmp = tmp_path_factory.mktemp("whole")
    one, chain = str(tmp / "one"), str(tmp / "chain")
    n = dc.discover_in_library(one, sample["fasta"], bam=sample["bam"])
    assert cases.run_in_library(["--analysis", "getCIGARindels", "--bamFile", sample["bam"], "--ref", sample["fasta"], "--outputFile", chain, "--quiet"]) == 0
    assert windows_in_library(["-i", chain + ".variants.txt", "--oneFile", chain + ".windows.txt", "--quiet"]) == 0
    return one, chain, n


def test_by_products_equal_the_two_tools_in_a_row(whole):
    one, chain, n = whole
    for ext in (".variants.txt", ".libraries.txt", ".windows.txt"):
        assert read(one + ext) == read(chain + ext) and read(one + ext), ext
    assert n == read(one + ".windows.txt").count("\n")


def test_the_sample_makes_the_windows_it_was_planted_for(sample, whole):
    one, _, _ = whole
    A = sample["targets"]["chrA"]
    variants = [l.split(" #")[0].split(" ") for l in read(one + ".variants.txt").split("\n") if l]
    # the homopolymer deletion: written at eight positions by the reads, one candidate behind the realignment
    in_run = [v for v in variants if v[0] == "chrA" and dc.RUN[0] - 2 <= int(v[1]) <= dc.RUN[1]]
    assert len(in_run) == 1 and in_run[0][2:] == ["-A"]
    cigar_starts = set()
    for tid, r, _ in sample["records"]:
        if tid == 0 and "1D" in r["cigar"] and r["pos"] < dc.RUN[1] < r["pos"] + dc.READ + 1:
            ops = r["cigar"].split("M")
            if ops[1].startswith("1D") and dc.RUN[0] <= r["pos"] + int(ops[0]) < dc.RUN[1]:
                cigar_starts.add(r["pos"] + int(ops[0]))
    assert len(cigar_starts) >= 6
    lines = read(one + ".windows.txt").split("\n")[:-1]
    by_tokens = {tuple(l.split(" ")[3:]): l.split(" ")[:3] for l in lines}
    tokens = lambda *t: tuple(t)
    assert by_tokens[tokens("900,+GAT")] == ["chrA", "840", "959"]
    assert by_tokens[tokens("1200,-" + A[1200:1202], "1215,+C")] == ["chrA", "1140", "1274"]                  # 15 apart: one window
    assert by_tokens[tokens("1500,-" + A[1500])] == ["chrA", "1440", "1560"] and tokens("1521,-" + A[1521:1524]) in by_tokens    # 21 apart: two
    B = sample["targets"]["chrB"]
    # the clamp (within 100 bases of the target's start the candidate tool, like the reference, names other letters than the deleted ones)
    assert [b for t, b in by_tokens.items() if len(t) == 1 and t[0].startswith("30,-") and len(t[0]) == 6] == [["chrB", "0", "91"]]
    assert tokens("1000,+TT") in by_tokens and tokens("1400,-" + B[1400:1404]) in by_tokens
    assert [l.split(" ")[0] for l in lines] == sorted(l.split(" ")[0] for l in lines)                          # BAM order of the targets
    assert len(lines) == 8


def test_options_pass_through_and_equal_the_chain(sample, whole, tmp_path):
    one, chain, _ = whole
    for k, (kw, args) in enumerate(((dict(min_dist=25, batch_candidates=3, host_convert=True), ["-m", "25"]), (dict(min_count=2), ["--minCount", "2"]),
                                    (dict(min_dist=25, min_count=1, max_count=12, events_cap=1), ["-m", "25", "--minCount", "1", "--maxCount", "12"]))):
        a, b = str(tmp_path / ("a%d" % k)), str(tmp_path / ("b%d" % k))
        dc.discover_in_library(a, sample["fasta"], bam=sample["bam"], **kw)
        assert read(a + ".variants.txt") == read(chain + ".variants.txt") and read(a + ".libraries.txt") == read(chain + ".libraries.txt")
        assert windows_in_library(["-i", chain + ".variants.txt", "--oneFile", b, "--quiet"] + args) == 0
        assert read(a + ".windows.txt") == read(b), kw
    wide, filtered = read(str(tmp_path / "a0.windows.txt")), read(str(tmp_path / "a1.windows.txt"))
    assert wide.count("\n") == 7 and " 1521,-" in wide.split("1500,-")[1].split("\n")[0]             # 21 apart: one window at --minDist 25
    # seen once: gone.  And chrA's last position with it: the filter, like the script, does not empty its buffer when the target changes
    assert "+TT" not in filtered and "1500,-" in filtered and "1521,-" not in filtered and "1400,-" in filtered


def test_region_run_over_two_files_equals_the_chain(sample, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    n = dc.discover_in_library(a, sample["fasta"], bam_list=sample["list"], tid="chrA", region="1,100-1,600")
    assert cases.run_in_library(["--analysis", "getCIGARindels", "--bamFiles", sample["list"], "--tid", "chrA", "--region", "1,100-1,600", "--ref", sample["fasta"],
                                 "--outputFile", b + ".variants.txt", "--quiet"]) == 0
    assert windows_in_library(["-i", b + ".variants.txt", "--oneFile", b + ".windows.txt", "--quiet"]) == 0
    assert read(a + ".variants.txt") == read(b + ".variants.txt") and read(a + ".windows.txt") == read(b + ".windows.txt")
    assert n == 3 and not __import__("os").path.exists(a + ".libraries.txt")


def test_stage_errors(sample, tmp_path):
    with pytest.raises(RuntimeError, match="Can extract the full set of indels from only BAM file at a time."):
        dc.discover_in_library(str(tmp_path / "x"), sample["fasta"], bam_list=sample["list"])
    with pytest.raises(RuntimeError, match="Cannot open file"):
        dc.discover_in_library(str(tmp_path / "x"), str(tmp_path / "none.fa"), bam=sample["bam"])
    with pytest.raises(RuntimeError, match="Cannot parse region"):
        dc.discover_in_library(str(tmp_path / "x"), sample["fasta"], bam=sample["bam"], tid="chrA", region="x")
