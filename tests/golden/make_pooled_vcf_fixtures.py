#!/usr/bin/env python3
"""Writes tests/golden/pooled_vcf.json: what the reference's own python/mergeOutputPooled.py (processPooledGLFFiles, getPercentiles) and
python/makeGenotypeLikelihoodFilePooled.py (makeGLF), with python/utils/Variant.py (Variant4), give for the inputs below.  These ARE
reference outputs.  Run only where the reference tree is present (oracle/Makefile names it; REFERENCE=<dir> overrides), like
make_vcf_candidates_fixtures.py:

    python tests/golden/make_pooled_vcf_fixtures.py

The scripts are Python 2.  They are loaded IN MEMORY exactly as make_vcf_candidates_fixtures.py loads its scripts (lib2to3 translates the
text, the result is exec'd into a module object; nothing of their text, translated or not, is written anywhere), with that script's
adjustment of Fasta.py and three more:

  * on the translated text of mergeOutputPooled.py, `numInds/2` becomes `numInds//2` — Python 2's meaning of python/mergeOutputPooled.py:407;
  * Python 2's `string.lower(s)` (FileUtils.py:29, FileUtils.py:43) no longer exists: an object with that function is put into the loaded
    FileUtils module's namespace under the name `string`;
  * likewise `string.count` and `string.upper` for the loaded VCFFile module, which makeGenotypeLikelihoodFilePooled.py imports.

Stored: `fasta` / `fai`, the reference the cases are written against; `percentiles`: [histogram, percentiles, result]; `variant4`: [REF, ALT,
type, offset, str] or [REF, ALT, null, null, [exception type, text]] for alleles of equal length; `merges`: per case the .glf.txt texts (every
text of the fixture is a list of indices into `lines`, see LinePool), the lines of the list file, the options, and either the VCF with the stderr and stdout texts or the exception's type and text; `glfs`: per case
the .glf.txt texts, the VCF of calls, the BAM names, and either the output with stderr and stdout or the exception.  Every path is
written as {DIR}/name.  Python 3 names some exceptions differently and words some messages differently: a comparison takes a NameError's
text exactly and any other exception by its type.

Two things are this recorder's, not the scripts'.  Where python/mergeOutputPooled.py:432-433 orders the chromosomes other than 1 ... 22, X, Y
by a Python-2 set — an order no Python 3 gives — the recorded VCF has those chromosomes' blocks of lines in ascending byte order, the
project's rule (host/glf_to_vcf.cpp); the lines inside a block are untouched.  And several variants at one position come out in the order
they were read (a Python-3 dict), where the script's order is a Python-2 dict's: a comparison takes the lines of one (chromosome, position)
as a sorted list.  Every est_freq and post_prob_variant cell has at most 12 significant digits, so that Python 3's repr prints the AF that
Python 2's str prints.  The .gz path is not recorded: Python 3's gzip hands the script bytes."""
import contextlib
import io
import json
import os
import random
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_vcf_candidates_fixtures as base          # noqa: E402  (its load() and reference_dir())

OUT = os.path.join(HERE, "pooled_vcf.json")
COLUMNS = ("msg index analysis_type tid lpos rpos center_position realigned_position was_candidate_in_window ref_all nref_all num_reads "
           "post_prob_variant qual est_freq logZ hapfreqs indidx msq numOffAll num_indel num_cover_forward num_cover_reverse "
           "num_unmapped_realigned var_coverage_forward var_coverage_reverse nBQT nmmBQT mLogBQ nMMLeft nMMRight glf").split()
HEADER = " ".join(COLUMNS) + "\n"


def load_scripts():
    base.load("utils/Fasta", [("int(pos)/idx.blen", "int(pos)//idx.blen")])
    base.load("utils/AnalyzeSequence")
    fileutils = base.load("utils/FileUtils")
    fileutils.string = types.SimpleNamespace(lower=lambda s: s.lower())
    variant = base.load("utils/Variant")
    vcffile = base.load("utils/VCFFile")
    vcffile.string = types.SimpleNamespace(count=lambda s, sub: s.count(sub), upper=lambda s: s.upper())
    merge = base.load("mergeOutputPooled", [("numInds/2", "numInds//2")])
    return variant, merge, base.load("makeGenotypeLikelihoodFilePooled")


# ---------------------------------------------------------------- the reference the cases are written against
def targets():
    rng = random.Random(2107)
    out = []
    for name, n in (("1", 520), ("2", 300), ("10", 260), ("X", 260), ("chrB", 240), ("chrA", 240), ("GL000207.1", 200)):
        seq = list("".join(rng.choice("ACGT") for _ in range(n)))
        if name == "1":
            seq[400:412] = "A" * 12                    # a homopolymer of 12
            seq[399], seq[412] = "C", "G"
        out.append((name, "".join(seq)))
    return out


# ---------------------------------------------------------------- .glf.txt lines
def row(**kw):
    d = dict(msg="ok", index="1", analysis_type="singlevariant", tid="1", lpos="40", rpos="160", center_position="100", realigned_position="100",
             was_candidate_in_window="1", ref_all="NA", nref_all="-AC", num_reads="20", post_prob_variant="0.99999", qual="NA", est_freq="0.25", logZ="-123.5",
             hapfreqs="NA", indidx="0", msq="NA", numOffAll="NA", num_indel="NA", num_cover_forward="4", num_cover_reverse="3", num_unmapped_realigned="NA",
             var_coverage_forward="5", var_coverage_reverse="6", nBQT="NA", nmmBQT="NA", mLogBQ="NA", nMMLeft="NA", nMMRight="NA", glf="0/0:-10.5;0/1:-2.25;1/1:-30")
    for k, v in kw.items():
        assert k in d, k
        d[k] = str(v)
    return " ".join(d[c] for c in COLUMNS) + "\n"


def site(index, tid, pos, var, prob="0.99999", freq="0.25", reads=(20, 14), pools=None, **kw):
    """the lines of one variant: one per pool, `reads` the pools' num_reads"""
    text = ""
    for b, nreads in enumerate(reads):
        text += row(index=index, tid=tid, realigned_position=pos, nref_all=var, post_prob_variant=prob, est_freq=freq, num_reads=nreads,
                    indidx=(pools[b] if pools else b), glf="0/0:-%d.5;0/1:-2.25;1/1:-3%d" % (10 + b, b), **kw)
    return text


def skipped(index, tid="1"):
    return row(msg="error_hapSize_error.", index=index, analysis_type="NA", tid=tid, lpos="500", rpos="620", center_position="NA", realigned_position="NA",
               was_candidate_in_window="NA", nref_all="NA", num_reads="NA", post_prob_variant="NA", est_freq="NA", logZ="NA", indidx="NA", num_cover_forward="NA",
               num_cover_reverse="NA", var_coverage_forward="NA", var_coverage_reverse="NA", glf="NA")


def dip(index, tid, pos, var, analysis="dip.map", **kw):
    return row(index=index, analysis_type=analysis, tid=tid, realigned_position=pos, nref_all=var, post_prob_variant="NA", est_freq="0.5", indidx="0",
               glf="*/*:-40.5;*/%s:-2.5;%s/%s:-30.5" % (var, var, var), **kw)


DEPTHS = site(90, "2", 30, "-T", prob="0.1", reads=(5, 4)) + site(91, "2", 60, "-T", prob="0.1", reads=(40, 30))     # two more depths: the range is [9, 70]


def merge_cases():
    c = []

    def add(name, *files, **kw):
        """files: texts (named f0.glf.txt ...) or (name, text) pairs; list: the list file's lines, {k} for file k"""
        fs = [f if isinstance(f, tuple) else ("f%d.glf.txt" % k, f) for k, f in enumerate(files)]
        opts = dict(numSamples=2, numBamFiles=2, maxHPLen=10, filterFR=False, filterQual=20)
        lst = kw.pop("list", None) or ["{%d}" % k for k in range(len(fs))]
        opts.update(kw)
        c.append(dict(name=name, files=[dict(name=n, text=t) for n, t in fs], list=lst, options=opts))

    H = HEADER
    add("two_sites_5bp_apart_both_stay_pass", H + site(1, "1", 100, "-AC") + site(2, "1", 105, "+G", prob="0.9995") + DEPTHS)
    add("filtered_beside_pass_gets_tc10", H + site(1, "1", 150, "-ACG", prob="0.9999") + site(2, "1", 155, "+TT", prob="0.995") + site(2, "1", 155, "-C", prob="0.9") +
        site(3, "1", 162, "-G", prob="0.9", freq="0.01") + site(4, "1", 300, "+A", prob="0.5") + DEPTHS)
    add("tie_in_qual_across_positions", H + site(1, "1", 306, "-A", prob="0.9999") + site(1, "1", 306, "+C", prob="0.3") + site(2, "1", 300, "-G", prob="0.9999") +
        site(2, "1", 300, "+T", prob="0.3") + site(3, "1", 312, "+GG", prob="0.9999") + site(3, "1", 312, "-T", prob="0.25") + DEPTHS)
    add("chain_of_close_sites", H + site(1, "1", 100, "-A", prob="0.999") + site(2, "1", 108, "-C", prob="0.99999") + site(2, "1", 108, "+C", prob="0.4") +
        site(3, "1", 116, "-G", prob="0.9995") + site(3, "1", 116, "+G", prob="0.5") + site(4, "1", 127, "-T", prob="0.9999") + site(4, "1", 127, "+T", prob="0.5") + DEPTHS)
    add("one_depth_value_only", H + site(1, "1", 100, "-AC") + site(2, "1", 200, "+G") + site(3, "2", 50, "-T"))
    add("header_only_file", H)
    add("chromosome_with_only_filtered_variants", H + site(1, "1", 100, "-AC") + site(2, "2", 100, "-T", prob="0.9") + site(3, "2", 150, "+G", freq="0.001") + DEPTHS)
    add("chromosome_names_outside_the_list", H + site(1, "chrB", 100, "-AC") + site(2, "X", 100, "+G") + site(3, "GL000207.1", 100, "-T") + site(4, "chrA", 120, "-G") +
        site(5, "10", 100, "+TT") + site(6, "2", 100, "-C") + site(7, "1", 100, "-A") + site(8, "chrA", 60, "+C") + DEPTHS)
    ns = H + site(1, "1", 100, "-AC", reads=(20, 0)) + site(2, "1", 200, "+G", reads=(0, 0)) + site(3, "1", 250, "-T", reads=(5, 4)) + site(4, "1", 280, "-T", prob="0.1", reads=(40, 30))
    add("numSamples_3_with_NS_1_is_not_s50", ns, numSamples=3)
    add("numSamples_4_with_NS_1_is_s50", ns, numSamples=4)
    fr = H + site(1, "1", 100, "-AC", var_coverage_forward="0") + site(2, "1", 200, "+G", var_coverage_reverse="0") + site(3, "1", 250, "-T") + DEPTHS
    add("filterFR", fr, filterFR=True)
    add("without_filterFR", fr)
    add("only_the_first_pools_var_coverage_counts", H + row(index=1, var_coverage_forward="3", var_coverage_reverse="2") +
        row(index=1, indidx="1", var_coverage_forward="0", var_coverage_reverse="0", num_cover_forward="7", num_cover_reverse="8", num_reads="11") + DEPTHS, filterFR=True)
    add("post_prob_variant_0.999_is_qual_29", H + site(1, "1", 100, "-AC", prob="0.999") + site(2, "1", 200, "+G", prob="0.99") + site(3, "1", 250, "-T", prob="0.9999999999") +
        site(4, "1", 280, "-T", prob="1") + site(5, "1", 320, "-T", prob="1.0000001") + site(6, "1", 350, "-TT", prob="0.990000000001") + DEPTHS)
    add("threshold_of_0.20", H + site(1, "1", 100, "-AC", prob="0.2") + site(2, "1", 200, "+G", prob="0.21") + site(3, "1", 250, "-T", prob="0.2000000001") + site(4, "1", 300, "-T") + DEPTHS)
    add("filterQual_10_and_30", H + site(1, "1", 100, "-AC", prob="0.95") + site(2, "1", 200, "+G", prob="0.85") + site(3, "1", 250, "-T", prob="0.9995") + DEPTHS, filterQual=10)
    add("filterQual_30", H + site(1, "1", 100, "-AC", prob="0.9995") + site(3, "1", 250, "-T", prob="0.99") + DEPTHS, filterQual=30)
    hp = H + site(1, "1", 400, "-A") + site(2, "1", 399, "-AA") + site(3, "1", 100, "-AC") + DEPTHS
    add("homopolymer", hp)
    add("homopolymer_maxHPLen_12", hp, maxHPLen=12)
    add("too_low_frequency", H + site(1, "1", 100, "-AC", freq="0.04") + site(2, "1", 200, "+G", freq="0.05") + site(3, "1", 250, "-T", freq="0.0499999") + DEPTHS)
    add("how_AF_is_written", H + site(1, "1", 100, "-AC", freq="1") + site(2, "1", 130, "+G", freq="0.5") + site(3, "1", 160, "-T", freq="0.123456789012") +
        site(4, "1", 190, "-T", freq="1e-05") + site(5, "1", 220, "-T", freq="0.0001") + site(6, "1", 250, "-T", freq="2.5e-1") + site(7, "1", 280, "-T", freq="1.5") +
        site(8, "1", 310, "-T", freq="100") + DEPTHS)
    add("deletions_and_insertions_from_the_fasta", H + site(1, "1", 100, "-ACGTA") + site(2, "1", 130, "+GATTACA") + site(3, "1", 160, "-T") + site(4, "2", 298, "-AC") +
        site(5, "2", 299, "+T") + DEPTHS)
    add("interleaved_dip_lines_NA_lines_short_last_group", H + site(1, "1", 100, "-AC") + dip(1, "1", 100, "-AC", "dip") + dip(1, "1", 100, "-AC") + skipped(2) +
        site(3, "1", 200, "+G") + row(index=4, realigned_position=250, nref_all="-T") + dip(4, "1", 250, "-T") + site(5, "1", 300, "-G") + skipped(6) + skipped(7) +
        DEPTHS + row(index=9, realigned_position=380, nref_all="-T"))
    add("a_group_ends_at_the_odd_line_and_the_rest_is_read_shifted", H + site(1, "1", 100, "-AC") + skipped(2) + row(index=3, realigned_position=200, nref_all="+G", indidx="1") +
        row(index=4, realigned_position=200, nref_all="-T", indidx="0") + row(index=4, realigned_position=250, nref_all="-T", indidx="1", post_prob_variant="0.1") +
        row(index=5, realigned_position=250, nref_all="-T", indidx="0", post_prob_variant="0.1") + DEPTHS)
    add("empty_line_ends_the_file", H + site(1, "1", 100, "-AC") + DEPTHS + "\n" + site(2, "1", 200, "+G"), H + site(3, "1", 300, "-G"))
    add("wrong_field_count", H + site(1, "1", 100, "-AC") + site(2, "1", 200, "+G").rsplit(" ", 1)[0] + "\n" + DEPTHS)
    add("one_field_too_many", H + site(1, "1", 100, "-AC") + row(index=2)[:-1] + " x\n" + DEPTHS)
    add("trailing_blanks_are_stripped", H + site(1, "1", 100, "-AC").replace("\n", "  \t\n") + DEPTHS)
    add("snp_line_above_0.2", H + site(1, "1", 100, "-AC") + site(2, "1", 200, "A=>C") + DEPTHS)
    add("snp_line_below_0.2_is_never_looked_at", H + site(1, "1", 100, "-AC") + site(2, "1", 200, "A=>C", prob="0.15") + DEPTHS)
    add("snp_line_on_a_chromosome_without_pass", H + site(1, "1", 100, "-AC") + site(2, "2", 200, "A=>C", prob="0.9") + DEPTHS)
    add("unrecognized_variant", H + site(1, "1", 100, "ACGT") + DEPTHS)
    add("ref_variant_first", H + site(1, "1", 100, "*REF") + DEPTHS)
    add("ref_variant_behind_another", H + site(1, "1", 100, "-AC") + site(2, "1", 200, "*REF") + DEPTHS)
    add("indidx_at_numBamFiles", H + site(1, "1", 100, "-AC") + site(2, "1", 200, "+G", pools=(0, 2)) + DEPTHS)
    add("numBamFiles_too_small", H + site(1, "1", 100, "-AC") + DEPTHS, numBamFiles=1)
    add("numBamFiles_3_on_two_pools", H + site(1, "1", 100, "-AC") + site(2, "1", 200, "+G") + DEPTHS, numBamFiles=3)
    add("position_differs_inside_a_group", H + site(1, "1", 100, "-AC") + row(index=2, realigned_position=200) + row(index=2, realigned_position=201, indidx="1") + DEPTHS)
    add("pools_in_the_wrong_order_only_warn", H + site(1, "1", 100, "-AC", pools=(1, 0)) + site(2, "1", 200, "+G", pools=(0, 0)) + DEPTHS)
    add("indidx_NA_inside_a_group", H + site(1, "1", 100, "-AC", pools=("NA", 1)) + DEPTHS)
    add("missing_column", H.replace(" var_coverage_reverse", "") + DEPTHS)
    add("missing_est_freq_column", H.replace(" est_freq", " estfreq") + site(1, "1", 100, "-AC") + DEPTHS)
    add("missing_est_freq_column_and_no_group", H.replace(" est_freq", " estfreq") + skipped(1))
    add("no_file_left", ("gone.glf.txt", None), ("empty.glf.txt", ""))
    add("missing_empty_and_inconsistent_files", H + site(1, "1", 100, "-AC") + DEPTHS, ("gone.glf.txt", None), ("empty.glf.txt", ""), H.replace("msg index", "index msg") + site(2, "1", 200, "+G"),
        H + site(3, "1", 300, "-G"), list=["{0} {1}", "", "  {2}\t{3}  ", "{4}"])
    add("later_group_replaces_the_earlier_one", H + site(1, "1", 100, "-AC", prob="0.9", reads=(7, 7)) + DEPTHS, H + site(1, "1", 100, "-AC", prob="0.99995", freq="0.5", reads=(9, 9)))
    add("unknown_chromosome", H + site(1, "1", 100, "-AC") + site(2, "chrZ", 100, "-T") + DEPTHS)
    add("unknown_chromosome_below_0.2", H + site(1, "1", 100, "-AC") + site(2, "chrZ", 100, "-T", prob="0.1") + DEPTHS)
    add("post_prob_not_a_number", H + site(1, "1", 100, "-AC", prob="high") + DEPTHS)
    add("num_reads_not_an_integer", H + site(1, "1", 100, "-AC", reads=("20.0", 14)) + DEPTHS)
    add("numSamples_0", H + site(1, "1", 100, "-AC") + DEPTHS, numSamples=0)
    add("numSamples_1", H + site(1, "1", 100, "-AC", freq="0.1") + site(2, "1", 200, "+G", freq="0.09", reads=(0, 0)) + DEPTHS, numSamples=1)
    return c


VCF_HEAD = "##fileformat=VCFv4.0\n##source=Dindel\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def rec(chrom, pos, ref, alt, qual="50", flt="PASS"):
    return "%s\t%s\t.\t%s\t%s\t%s\t%s\tAF=0.25;NS=2\n" % (chrom, pos, ref, alt, qual, flt)


def glf_cases():
    c = []

    def add(name, vcf, *files, **kw):
        fs = [f if isinstance(f, tuple) else ("g%d.glf.txt" % k, f) for k, f in enumerate(files)]
        c.append(dict(name=name, vcf=vcf, vcf_name=kw.get("vcf_name", "calls.vcf"), files=[dict(name=n, text=t) for n, t in fs],
                      list=kw.get("list") or ["{%d}" % k for k in range(len(fs))], bams=kw.get("bams", ["poolA.bam extra words", "/data/poolB.bam"])))

    H = HEADER
    calls = VCF_HEAD + rec("1", 100, "GAC", "G") + rec("1", 200, "T", "TG", "9", "q20") + rec("1", 250, "CT", "C", "10", "q20") + rec("1", 300, "AG", "A", "99", "q20;tc10") + \
        rec("2", 50, "A", "ATT", "10.5", "q20") + rec("2", 80, "AC", "A", "30", "hp10")
    body = site(1, "1", 100, "-AC") + site(2, "1", 200, "+G") + site(3, "1", 250, "-T") + site(4, "1", 300, "-G") + site(5, "2", 50, "+TT") + site(6, "2", 80, "-C") + site(7, "2", 100, "-AC")
    add("q20_with_qual_9_and_10", calls, H + body)
    add("group_of_the_wrong_length", calls, H + site(1, "1", 100, "-AC", reads=(20, 14, 3)) + site(3, "1", 250, "-T", reads=(20,)) + site(5, "2", 50, "+TT"))
    add("pooled_and_diploid_lines_of_one_window", calls, H + site(1, "1", 100, "-AC") + dip(1, "1", 100, "-AC", "dip") + site(3, "1", 250, "-T") + dip(3, "1", 251, "-T") + site(5, "2", 50, "+TT"))
    add("dip_map_line_of_a_called_site", calls, H + dip(1, "1", 100, "-AC"), bams=["only.bam"])
    add("dip_map_line_of_a_site_not_called", calls, H + dip(1, "1", 400, "-AC") + site(3, "1", 250, "-T", reads=(20,)), bams=["only.bam"])
    add("two_files_with_the_same_first_position", calls, H + site(1, "1", 100, "-AC"), H + skipped(1) + site(2, "2", 100, "-AC"))
    add("files_in_the_order_of_their_first_position", calls, H + site(5, "2", 50, "+TT") + site(3, "1", 250, "-T"), H + skipped(9) + site(1, "1", 100, "-AC"), H + skipped(1) + site(1, "1", 40, "-A"))
    add("na_lines_and_na_groups", calls, H + skipped(1) + site(1, "1", 100, "-AC") + skipped(2) + skipped(2) + row(index=3, realigned_position="250", nref_all="NA") + site(3, "1", 250, "-T") + skipped(4))
    add("position_NA_with_a_variant_on_a_called_chromosome", calls, H + site(1, "1", 100, "-AC") + row(index=3, realigned_position="NA", nref_all="-T") + site(3, "1", 250, "-T"))
    add("position_NA_with_a_variant_on_another_chromosome", calls, H + site(1, "1", 100, "-AC") + row(index=3, tid="7", realigned_position="NA", nref_all="-T") + site(3, "1", 250, "-T"))
    add("missing_glf_file", calls, H + body, ("gone.glf.txt", None))
    add("list_line_with_several_words", calls, H + body, H + site(1, "1", 40, "-A"), list=["{0} {1}"])
    add("wrong_field_count", calls, H + site(1, "1", 100, "-AC") + site(3, "1", 250, "-T").rsplit(" ", 1)[0] + "\n")
    add("header_only_glf", calls, H)
    add("empty_line_ends_the_file", calls, H + site(1, "1", 100, "-AC") + "\n" + site(3, "1", 250, "-T"))
    add("glf_cell_without_colon", calls, H + site(1, "1", 100, "-AC").replace("0/1:-2.25", "0/1"))
    add("glf_cell_without_1_1", calls, H + site(1, "1", 100, "-AC").replace(";1/1:-30", "").replace(";1/1:-31", ""))
    add("indidx_beyond_the_bam_names", calls, H + site(1, "1", 100, "-AC", pools=(0, 2)))
    add("indidx_negative", calls, H + site(1, "1", 100, "-AC", pools=(-1, -2)))
    add("comma_in_alt", VCF_HEAD + rec("1", 100, "GAC", "G,GA"), H + body)
    add("comma_in_alt_of_a_filtered_record", VCF_HEAD + rec("1", 100, "GAC", "G,GA", flt="hp10") + rec("1", 250, "CT", "C"), H + body)
    add("same_variant_twice", VCF_HEAD + rec("1", 100, "GAC", "G") + rec("1", 100, "GAC", "G", "10", "q20"), H + body)
    add("same_variant_from_two_records", VCF_HEAD + rec("1", 100, "GAC", "G") + rec("1", 99, "TGAC", "TG"), H + body)
    add("not_a_vcf4_insertion", VCF_HEAD + rec("1", 100, "G", "TG"), H + body)
    add("snp_record", VCF_HEAD + rec("1", 100, "GAC", "GAT") + rec("1", 250, "C", "T"), H + site(1, "1", 102, "C=>T") + site(2, "1", 250, "C=>T") + site(3, "1", 100, "C=>T"))
    add("multi_snp_record", VCF_HEAD + rec("1", 100, "GAC", "GTT"), H + body)
    add("alt_equal_to_ref", VCF_HEAD + rec("1", 100, "GAC", "GAC"), H + body)
    add("qual_not_a_number_in_a_q20_record", VCF_HEAD + rec("1", 100, "GAC", "G", ".", "q20"), H + body)
    add("qual_not_a_number_in_a_pass_record", VCF_HEAD + rec("1", 100, "GAC", "G", "."), H + body)
    add("vcf_without_filter_column", VCF_HEAD.replace("\tFILTER", "") + "1\t100\t.\tGAC\tG\t50\tAF=0.25\n", H + body)
    add("vcf_line_with_a_wrong_field_count", VCF_HEAD + rec("1", 100, "GAC", "G") + "1\t250\t.\tCT\tC\t50\tPASS\n", H + body)
    add("vcf_ends_at_an_empty_line", VCF_HEAD + rec("1", 100, "GAC", "G") + "\n" + rec("1", 250, "CT", "C"), H + body)
    add("no_calls", VCF_HEAD, H + body)
    add("call_file_not_named_vcf", calls, H + body, vcf_name="calls.txt")
    add("empty_line_in_the_bam_list", calls, H + body, bams=["poolA.bam", "", "poolB.bam"])
    add("empty_line_in_the_glf_list", calls, H + body, list=["{0}", ""])
    return c


def variant4_pairs():
    import itertools
    alleles = ["".join(t) for n in range(1, 4) for t in itertools.product("AC", repeat=n)]
    return [(r, a) for r in alleles for a in alleles if len(r) == len(a)] + [("GATTACA", "GATTACA"), ("GATTACA", "GATTACT"), ("GATTACA", "CATTACA"), ("GATTACA", "GACTACT"), ("", "")]


PERCENTILES = [({20: 5}, [1, 99]), ({}, [1, 99]), ({9: 1, 34: 3, 70: 1}, [1, 99]), ({0: 2, 5: 200, 9: 1}, [1, 99]), ({1: 1, 2: 1, 3: 1, 4: 1, 5: 1, 6: 1, 7: 1, 8: 1, 9: 1, 10: 1}, [1, 5, 10, 25, 50, 75, 90, 95, 99]),
               ({3: 1000, 4: 1, 5: 1}, [1, 99]), ({3: 1, 4: 1000, 5: 1, 6: 1}, [1, 99]), ({10: 98, 20: 1, 30: 1}, [1, 99]), ({10: 1, 20: 1}, [50, 50, 50]), ({0: 1}, [1, 99])]


def put(d, name, text):
    with open(os.path.join(d, name), "w", newline="") as f:
        f.write(text)


def reorder_other_chromosomes(vcf):
    """see the docstring: the blocks of the chromosomes other than 1 ... 22, X, Y in ascending byte order"""
    lines = vcf.split("\n")[:-1]
    head = [l for l in lines if l.startswith("#")]
    named = [str(k) for k in range(1, 23)] + ["X", "Y"]
    blocks = []
    for l in lines[len(head):]:
        chrom = l.split("\t")[0]
        if not blocks or blocks[-1][0] != chrom:
            blocks.append((chrom, []))
        blocks[-1][1].append(l)
    assert len({b[0] for b in blocks}) == len(blocks)
    first = [b for b in blocks if b[0] in named]
    assert [b[0] for b in first] == sorted((b[0] for b in first), key=named.index)
    other = sorted((b for b in blocks if b[0] not in named), key=lambda b: b[0].encode())
    return "".join(l + "\n" for l in head + [l for b in first + other for l in b[1]])


def run(fn, d, rec, out_name):
    err, so = io.StringIO(), io.StringIO()
    sub = lambda s: s.replace(d, "{DIR}")
    try:
        with contextlib.redirect_stderr(err), contextlib.redirect_stdout(so):
            fn()
    except Exception as e:                            # whatever kills the script
        rec["error"] = dict(type=type(e).__name__, text=sub(str(e)))
    else:
        rec["output"] = sub(open(os.path.join(d, out_name)).read())
    rec["stderr"], rec["stdout"] = sub(err.getvalue()), sub(so.getvalue())


class LinePool:
    """Every text of the fixture as a list of indices into one table of distinct lines (`lines`): the rows that many cases share are stored
    once.  A line of as many cells as the default row (`default_row`) is stored as [column, cell, column, cell, ...] of the cells that differ
    from it; any other line as it is.  unpack() in tests/test_pooled_vcf_cpu.py is the inverse, and pack() checks that it is."""
    def __init__(self):
        self.default = row()[:-1].split(" ")
        self.lines, self.index = [], {}

    def entry(self, line):
        cells = line[:-1].split(" ")
        if line.endswith("\n") and len(cells) == len(self.default) and "\t" not in line:
            return [x for i, c in enumerate(cells) if c != self.default[i] for x in (i, c)]
        return line

    def pack(self, text):
        ids = []
        for line in text.splitlines(keepends=True):
            if line not in self.index:
                self.index[line] = len(self.lines)
                self.lines.append(self.entry(line))
            ids.append(self.index[line])
        assert "".join(self.text_of(i) for i in ids) == text
        return ids

    def text_of(self, i):
        e = self.lines[i]
        if isinstance(e, str):
            return e
        cells = list(self.default)
        for k in range(0, len(e), 2):
            cells[e[k]] = e[k + 1]
        return " ".join(cells) + "\n"


def write_packed(out):
    pool = LinePool()
    for c in out["merges"] + out["glfs"]:
        for f in c["files"]:
            f["text"] = None if f["text"] is None else pool.pack(f["text"])
        for k in ("vcf", "output", "stderr", "stdout"):
            if k in c:
                c[k] = pool.pack(c[k])
    out["default_row"], out["lines"] = pool.default, pool.lines
    dumps = lambda x: json.dumps(x, sort_keys=True, separators=(",", ":"))
    with open(OUT, "w") as f:                         # one case per line
        f.write("{\n")
        for k in sorted(out):
            v = out[k]
            if k in ("merges", "glfs", "lines"):
                step = 25 if k == "lines" else 1
                body = ",\n".join(dumps(v[i:i + step])[1:-1] for i in range(0, len(v), step))
                f.write('"%s":[\n%s\n]' % (k, body))
            else:
                f.write('"%s":%s' % (k, dumps(v)))
            f.write(",\n" if k != sorted(out)[-1] else "\n")
        f.write("}\n")
    json.load(open(OUT))


def main():
    variant, merge, glf = load_scripts()
    out = dict(variant4=[], percentiles=[], merges=[], glfs=[])
    for hist, pct in PERCENTILES:
        out["percentiles"].append([sorted(hist.items()), pct, merge.getPercentiles(dict(hist), list(pct))])
    for ref, alt in variant4_pairs():
        try:
            v = variant.Variant4(ref=ref, alt=alt)
            out["variant4"].append([ref, alt, v.type, v.offset, v.str])
        except Exception as e:
            out["variant4"].append([ref, alt, None, None, [type(e).__name__, str(e)]])
    tg = targets()
    out["fasta"], out["fai"] = base.fasta_and_index(tg)
    for c in merge_cases():
        with tempfile.TemporaryDirectory() as d:
            put(d, "ref.fa", out["fasta"])
            put(d, "ref.fa.fai", out["fai"])
            for f in c["files"]:
                if f["text"] is not None:
                    put(d, f["name"], f["text"])
            put(d, "list.txt", "".join(l.format(*[os.path.join(d, f["name"]) for f in c["files"]]) + "\n" for l in c["list"]))
            o = c["options"]
            run(lambda: merge.processPooledGLFFiles(glfFilesFile=os.path.join(d, "list.txt"), maxHPLen=o["maxHPLen"], refFile=os.path.join(d, "ref.fa"),
                                                    outputVCFFile=os.path.join(d, "out.vcf"), doNotFilterOnFR=not o["filterFR"], filterQual=o["filterQual"],
                                                    numSamples=o["numSamples"], numBamFiles=o["numBamFiles"]), d, c, "out.vcf")
            if "output" in c:
                c["output"] = reorder_other_chromosomes(c["output"])
            out["merges"].append(c)
    for c in glf_cases():
        with tempfile.TemporaryDirectory() as d:
            for f in c["files"]:
                if f["text"] is not None:
                    put(d, f["name"], f["text"])
            put(d, "list.txt", "".join(l.format(*[os.path.join(d, f["name"]) for f in c["files"]]) + "\n" for l in c["list"]))
            put(d, "bams.txt", "".join(b + "\n" for b in c["bams"]))
            put(d, c["vcf_name"], c["vcf"])
            run(lambda: glf.makeGLF(inputGLFFiles=os.path.join(d, "list.txt"), outputFile=os.path.join(d, "out.txt"), callFile=os.path.join(d, c["vcf_name"]),
                                    bamfilesFile=os.path.join(d, "bams.txt")), d, c, "out.txt")
            out["glfs"].append(c)
    write_packed(out)
    print("wrote %s: %d merges (%d raise), %d glfs (%d raise)" % (OUT, len(out["merges"]), sum("error" in c for c in out["merges"]), len(out["glfs"]),
                                                                sum("error" in c for c in out["glfs"])))


if __name__ == "__main__":
    sys.exit(main())
