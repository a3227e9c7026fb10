#!/usr/bin/env python3
"""Writes tests/golden/vcf_candidates.json: what the reference's own python/convertVCFToDindel.py (convert) and python/utils/Variant.py
(Variant4) give for the inputs below.  These ARE reference outputs.  Run only where the reference tree is present (oracle/Makefile names
it; REFERENCE=<dir> overrides), like make_windows_fixtures.py:

    python tests/golden/make_vcf_candidates_fixtures.py

The scripts are Python 2.  utils/Fasta.py, utils/AnalyzeSequence.py, utils/FileUtils.py, utils/Variant.py, utils/VCFFile.py and
convertVCFToDindel.py are loaded IN MEMORY: lib2to3's RefactoringTool.refactor_string translates the text and the result is exec'd into a
module object that the later ones import by its name; nothing of their text, translated or not, is written anywhere.  Two adjustments:

  * on the translated text of Fasta.py, `int(pos)/idx.blen` becomes `int(pos)//idx.blen` — Python 2's meaning of that line
    (python/utils/Fasta.py:41; under Python 3 the true division hands seek() a float);
  * Python 2's `string.count(s, sub)` and `string.upper(s)` (python/utils/VCFFile.py:117, python/utils/VCFFile.py:142) no longer exist: an
    object with these two functions is put into the loaded VCFFile module's namespace under the name `string`.  No text changes.

Stored: (a) `variant4`: [REF, ALT, type, offset, str] or [REF, ALT, null, null, raised text] for every pair over {A, C} with lengths
1 ... 4 each and unequal lengths, and hand-picked longer pairs in repeats; (b) `conversions`: per case the VCF texts, minQual, and either
the output lines with the stderr and stdout texts, or the exception's type and text (what is left in the output file then is not part of
the contract).  Python 3 names some exceptions differently from Python 2 (IOError is OSError) and words some messages differently;
a comparison takes a NameError's text exactly and any other exception by its type.  `fasta` and `fai` are the reference the cases
are written against.  The .gz path is not recorded here: Python 3's gzip hands the script bytes."""
import contextlib
import io
import itertools
import json
import os
import random
import re
import sys
import tempfile
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "vcf_candidates.json")


def reference_dir():
    if os.environ.get("REFERENCE"):
        return os.environ["REFERENCE"]
    return re.search(r"^REFERENCE \?= *(\S+)", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M).group(1)


def load(path, substitutions=()):
    """the script at python/<path>.py as a module object registered under its bare name"""
    name = os.path.basename(path)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from lib2to3 import refactor
        tool = refactor.RefactoringTool(refactor.get_fixers_from_package("lib2to3.fixes"))
        text = open(os.path.join(reference_dir(), "python", path + ".py")).read()
        text = str(tool.refactor_string(text, name))
    for old, new in substitutions:
        assert text.count(old) == 1, (name, old)
        text = text.replace(old, new)
    mod = types.ModuleType(name)
    sys.modules[name] = mod
    exec(compile(text, name, "exec"), mod.__dict__)
    return mod


def load_scripts():
    load("utils/Fasta", [("int(pos)/idx.blen", "int(pos)//idx.blen")])
    load("utils/AnalyzeSequence")
    load("utils/FileUtils")
    variant = load("utils/Variant")
    vcffile = load("utils/VCFFile")
    vcffile.string = types.SimpleNamespace(count=lambda s, sub: s.count(sub), upper=lambda s: s.upper())
    return variant, load("convertVCFToDindel")


# ---------------------------------------------------------------- the reference the cases are written against
LINE = 50


def targets():
    rng = random.Random(1906)
    chr1 = list("".join(rng.choice("ACGT") for _ in range(430)))
    chr1[100:112] = "A" * 12                           # a homopolymer
    chr1[99], chr1[112] = "C", "G"
    chr1[200:214] = "CA" * 7                           # a dinucleotide repeat
    chr1[199], chr1[214] = "T", "G"
    chr1[300:303] = "acg"                              # lower case stays lower case
    chr2 = "".join(rng.choice("ACGT") for _ in range(175))
    return [("chr1", "".join(chr1)), ("chr2", chr2)]


def fasta_and_index(tg):
    fa, fai = "", ""
    for name, seq in tg:
        fa += ">%s\n" % name
        fai += "%s\t%d\t%d\t%d\t%d\n" % (name, len(seq), len(fa), LINE, LINE + 1)
        fa += "".join(seq[i:i + LINE] + "\n" for i in range(0, len(seq), LINE))
    return fa, fai


TG = dict(targets())
V4 = ('##fileformat=VCFv4.0\n##source=test\n##INFO=<ID=DP,Number=1,Type=Integer,Description="Total Depth">\n'
      '##INFO=<ID=AF,Number=.,Type=Float,Description="Allele Frequency, per ALT">\n##FILTER=<ID=q10,Description="Quality below 10">\n'
      '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n')
V3 = ('##fileformat=VCFv3.3\n##INFO=DP,1,Integer,"Total Depth"\n##INFO=HM,.,Integer,"HapMap membership"\n##FILTER=q10,"Quality below 10"\n'
      '##FORMAT=GT,1,String,"Genotype"\n##FORMAT=HQ,.,Integer,"Haplotype Quality"\n')
COLS = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
COLS_S = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tNA001\tNA002\n"


def dele(chrom, pos1, n, qual="50", extra_alt="", tail="PASS\tDP=10"):
    """a VCF4 deletion of n bases behind the base at one-based pos1"""
    ref = TG[chrom][pos1 - 1:pos1 + n]
    return "%s\t%d\t.\t%s\t%s%s\t%s\t%s\n" % (chrom, pos1, ref, ref[0], extra_alt, qual, tail)


def ins(chrom, pos1, seq, qual="50", tail="PASS\tDP=10"):
    ref = TG[chrom][pos1 - 1]
    return "%s\t%d\t.\t%s\t%s\t%s\t%s\n" % (chrom, pos1, ref, ref + seq, qual, tail)


def conversion_cases():
    c = []
    add = lambda name, *vcfs, **kw: c.append(dict(name=name, vcfs=list(vcfs), minQual=kw.get("minQual", 1.0)))
    add("plain", V4 + COLS + dele("chr1", 20, 2) + ins("chr1", 60, "GG") + dele("chr1", 105, 1) + dele("chr1", 205, 2) + ins("chr2", 33, "T") + dele("chr2", 150, 5))
    # several ALTs: <DEL>, one as long as REF, a deletion and an insertion off one REF
    r = TG["chr1"][39:43]
    add("multi_alt", V4 + COLS + "chr1\t40\t.\t%s\t<DEL>,%s,%s,%s\t30\tPASS\tDP=3\n" % (r, r[0] + "T" + r[2:], r[0] + r[3:], r[:2] + "TTT" + r[2:]) + dele("chr1", 70, 1, extra_alt=",<DEL>"))
    quals = V4 + COLS + dele("chr1", 20, 1, qual=".") + dele("chr1", 30, 1, qual="9.99") + dele("chr1", 40, 1, qual="10") + dele("chr1", 50, 1, qual="10.5") + \
        dele("chr1", 60, 1, qual="1e2") + dele("chr1", 70, 1, qual="0") + dele("chr1", 80, 1, qual="1")
    add("qual_default_minQual", quals)
    add("qual_minQual_10", quals, minQual=10.0)
    # REF that is not the FASTA's (the line is still written); lower case in the FASTA is not upper-cased, so an upper-case REF differs
    add("ref_mismatch", V4 + COLS + "chr1\t20\t.\tGGG\tG\t50\tPASS\tDP=1\n" + "chr1\t301\t.\tACG\tA\t50\tPASS\tDP=1\n" + "chr1\t301\t.\tacg\ta\t50\tPASS\tDP=1\n" +
        "chr2\t174\t.\t%sAAAA\t%s\t50\tPASS\tDP=1\n" % (TG["chr2"][173], TG["chr2"][173]))
    add("two_files", V4 + COLS + dele("chr2", 20, 2) + dele("chr1", 20, 2), V3 + COLS + ins("chr1", 90, "A", tail="0\tDP=1") + dele("chr2", 20, 2, tail="q10\tDP=1"))
    add("blank_line_in_the_middle", V4 + COLS + dele("chr1", 20, 2) + "\n" + dele("chr1", 60, 2))
    add("blank_line_then_second_file", V4 + COLS + dele("chr1", 20, 2) + "\n" + dele("chr1", 60, 2), V4 + COLS + dele("chr2", 60, 2))
    add("short_line", V4 + COLS + dele("chr1", 20, 2) + "chr1\t30\t.\tAC\tA\t50\n" + dele("chr1", 60, 2))
    add("one_field_short_of_the_last_column", V4 + COLS + dele("chr1", 20, 2) + "chr1\t30\t.\tAC\tA\t50\tPASS\n" + dele("chr1", 60, 2))
    add("one_field_short_with_samples", V4 + COLS_S + dele("chr1", 20, 2, tail="PASS\tDP=1\tGT\t0/1\t1/1") + dele("chr1", 30, 2, tail="PASS\tDP=1\tGT\t0/1") + dele("chr1", 60, 2))
    add("v3_header", V3 + COLS + dele("chr1", 20, 2, tail="0\tDP=1;HM") + ins("chr2", 40, "AC", tail="q10\tDP=1"))
    add("v4_header_spaces_and_case", '##fileformat=VCFv4.1\n##INFO=<id=DP, number=1,Type =Integer,description="x, y, z">\n##FILTER=<ID=q10,Description="d">\n' + COLS + dele("chr1", 20, 2))
    add("no_info_lines_warns", "##fileformat=VCFv4.0\n" + COLS + dele("chr1", 20, 2))
    add("incomplete_description", '##fileformat=VCFv4.0\n##INFO=<ID=DP,Number=1,Type=Integer,Description="Total Depth>\n' + COLS + dele("chr1", 20, 2))
    add("incomplete_filter_description", '##fileformat=VCFv4.0\n##FILTER=<ID=q10,Description=Quality>\n' + COLS + dele("chr1", 20, 2))
    add("incorrect_description", '##fileformat=VCFv4.0\n##INFO=ID=DP,Number=1,Type=Integer,Description="Total Depth"\n' + COLS + dele("chr1", 20, 2))
    add("no_type_in_info", '##fileformat=VCFv4.0\n##INFO=<ID=DP,Number=1,Kind=Integer,Description="Total Depth">\n' + COLS + dele("chr1", 20, 2))
    add("no_number_in_format", '##fileformat=VCFv4.0\n##FORMAT=<ID=GT,Type=String,Description="Genotype">\n' + COLS + dele("chr1", 20, 2))
    add("info_of_two_fields", '##fileformat=VCFv4.0\n##INFO=<ID=DP,Number=1,Description="Total Depth">\n' + COLS + dele("chr1", 20, 2))
    add("v3_info_id_twice", V3 + '##INFO=DP,1,Integer,"again"\n' + COLS + dele("chr1", 20, 2))
    add("v3_number_not_an_integer", '##fileformat=VCFv3.3\n##INFO=DP,one,Integer,"Total Depth"\n' + COLS + dele("chr1", 20, 2))
    add("unknown_version", "##fileformat=VCFv5.0\n" + COLS + dele("chr1", 20, 2))
    add("fileformat_without_vcf", "##fileformat=BCF2\n" + COLS + dele("chr1", 20, 2))
    add("description_in_front_of_fileformat", '##INFO=<ID=DP,Number=1,Type=Integer,Description="Total Depth">\n##fileformat=VCFv4.0\n' + COLS + dele("chr1", 20, 2))
    add("missing_main_column", V4 + "#CHROM\tPOS\tID\tREF\tALT\tFILTER\tINFO\n" + "chr1\t20\t.\tAC\tA\tPASS\tDP=1\n")
    add("missing_info_column", V4 + "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\n" + "chr1\t20\t.\tAC\tA\t50\tPASS\n")
    add("missing_fileformat", "##source=test\n" + COLS + dele("chr1", 20, 2))
    add("missing_fileformat_and_no_full_line", "##source=test\n" + COLS + "chr1\t20\t.\tAC\n")
    add("missing_header_line", V4 + dele("chr1", 20, 2))
    add("empty_file", "")
    add("lines_in_front_of_the_header_are_passed_over", V4 + dele("chr1", 20, 2) + "#comment\n" + COLS + dele("chr1", 60, 2))
    add("columns_in_another_order_and_labels_split_on_blanks", V4 + "#CHROM POS  ID\tALT REF QUAL FILTER INFO\n" + "chr1\t20\t.\t%s\t%s\t50\tPASS\tDP=1\n" % (TG["chr1"][19], TG["chr1"][19:22]))
    add("data_lines_split_on_tabs_only", V4 + COLS + "chr1 20 . AC A 50 PASS DP=1\n" + dele("chr1", 60, 2))
    add("sample_columns", V4 + COLS_S + dele("chr1", 20, 2, tail="PASS\tDP=1\tGT\t0/1\t1/1") + ins("chr1", 60, "G", tail="q10;s50\tDP=1;AF=0.5\tGT\t0/1\t./."))
    add("variant4_error_in_the_middle", V4 + COLS + dele("chr1", 20, 2) + "chr1\t30\t.\t%s\tT%s\t50\tPASS\tDP=1\n" % (TG["chr1"][29], TG["chr1"][29]) + dele("chr1", 60, 2))
    add("alt_dot_against_a_longer_ref", V4 + COLS + "chr1\t20\t.\t%s\t.\t50\tPASS\tDP=1\n" % TG["chr1"][19:21])
    add("alt_dot_against_one_base", V4 + COLS + "chr1\t20\t.\t%s\t.\t50\tPASS\tDP=1\n" % TG["chr1"][19] + dele("chr1", 60, 2))
    add("unknown_target", V4 + COLS + dele("chr1", 20, 2) + "chrX\t30\t.\tAC\tA\t50\tPASS\tDP=1\n")
    add("pos_not_a_number", V4 + COLS + dele("chr1", 20, 2) + "chr1\tx30\t.\tAC\tA\t50\tPASS\tDP=1\n")
    add("qual_not_a_number", V4 + COLS + dele("chr1", 20, 2) + "chr1\t30\t.\tAC\tA\thigh\tPASS\tDP=1\n")
    add("pos_with_blanks_around", V4 + COLS + "chr1\t 20 \t.\t%s\t%s\t 50 \tPASS\tDP=1\n" % (TG["chr1"][19:22], TG["chr1"][19]))
    add("low_qual_record_is_still_checked", V4 + COLS + "chr1\t20\t.\tGGG\tG\t0.5\tPASS\tDP=1\n" + "chrX\t30\t.\tAC\tA\t0\tPASS\tDP=1\n")
    add("no_newline_at_the_end", V4 + COLS + dele("chr1", 20, 2) + dele("chr1", 60, 2)[:-1])
    add("first_base_and_last_base", V4 + COLS + dele("chr1", 1, 2) + dele("chr2", 1, 1) + dele("chr1", 428, 2) + ins("chr2", 175, "AC"))
    add("repeats_written_where_the_vcf_has_them", V4 + COLS + dele("chr1", 100, 1) + dele("chr1", 104, 3) + dele("chr1", 111, 1) + dele("chr1", 200, 2) + dele("chr1", 204, 4) +
        "chr1\t201\t.\tCACAC\tCAC\t50\tPASS\tDP=1\n" + "chr1\t201\t.\tCAC\tCACAC\t50\tPASS\tDP=1\n")
    return c


LONGER_PAIRS = [("CAAAAAAT", "CAAAAT"), ("CAAAAT", "CAAAAAAT"), ("TCACACACAG", "TCACACAG"), ("TCACACAG", "TCACACACACAG"), ("GACGACGACGT", "GACGT"), ("GT", "GACGACGT"),
                ("ACGTACGT", "ACGT"), ("ACGT", "ACGTACGT"), ("AAAAAAAA", "AAA"), ("AAA", "AAAAAAAA"), ("ATTTG", "ATG"), ("ATG", "ATTTG"), ("ACCCT", "AT"), ("TC", "TTTC"),
                ("ACG", "ATCG"), ("AG", "ACCG"), ("ACGT", "AT"), ("AT", "A"), ("A", "TA"), ("AC", "GTC"), ("AAC", "C"), ("GATTACA", "GA"), ("GA", "GATTACA"),
                ("CTTTTTTTTTTC", "CTC"), ("ACACACAC", "ACAC"), ("ACAC", "ACACACAC"), ("TAGCTAGCTAGC", "TAGC"), ("A", ""), ("", "A"), ("AT", "."), ("<DEL>", "A")]


def main():
    variant, convert = load_scripts()
    out = dict(variant4=[], conversions=[])
    alleles = ["".join(t) for n in range(1, 5) for t in itertools.product("AC", repeat=n)]
    for ref, alt in [(r, a) for r in alleles for a in alleles if len(r) != len(a)] + LONGER_PAIRS:
        try:
            v = variant.Variant4(ref=ref, alt=alt)
            out["variant4"].append([ref, alt, v.type, v.offset, v.str])
        except NameError as e:
            out["variant4"].append([ref, alt, None, None, str(e)])
    tg = targets()
    out["fasta"], out["fai"] = fasta_and_index(tg)
    for c in conversion_cases():
        with tempfile.TemporaryDirectory() as d:
            fa = os.path.join(d, "ref.fa")
            open(fa, "w").write(out["fasta"])
            open(fa + ".fai", "w").write(out["fai"])
            names = []
            for k, text in enumerate(c["vcfs"]):
                names.append(os.path.join(d, "in%d.vcf" % k))
                open(names[-1], "w", newline="").write(text)
            outp = os.path.join(d, "out.txt")
            err, so = io.StringIO(), io.StringIO()
            rec = dict(c)
            try:
                with contextlib.redirect_stderr(err), contextlib.redirect_stdout(so):
                    convert.convert(inputVCFFile=",".join(names), outputVariantFile=outp, parameters=dict(refFile=fa, minQual=c["minQual"]))
            except Exception as e:              # whatever kills the script
                rec["error"] = dict(type=type(e).__name__, text=str(e))
                rec["stdout"] = so.getvalue()
            else:
                rec["lines"] = open(outp).read().split("\n")[:-1]
                rec["stderr"], rec["stdout"] = err.getvalue(), so.getvalue()
            out["conversions"].append(rec)
    json.dump(out, open(OUT, "w"), indent=0, sort_keys=True)
    print("wrote %s: %d Variant4 pairs, %d conversions (%d raise)" % (OUT, len(out["variant4"]), len(out["conversions"]), sum("error" in c for c in out["conversions"])))


if __name__ == "__main__":
    sys.exit(main())
