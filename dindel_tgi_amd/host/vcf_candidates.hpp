// vcf_candidates.hpp — candidate indels from a VCF of known sites: VCF records -> `tid pos variant` lines (zero-based, no counts; what
// `dindel_candidates --analysis realignCandidates` reads).  Restates the reference's Python-2 script python/convertVCFToDindel.py with the
// parts of python/utils/VCFFile.py, python/utils/Variant.py and python/utils/Fasta.py it runs, rule for rule; plain C++, no GPU: the
// step is text and integer work per record.  A file is taken as bytes, as Python 2 takes it: only '\n' ends a line, a '\r' is a letter.
//
//   files and order      python/convertVCFToDindel.py:12-19   the output file is opened, then the FASTA and its index, then the VCFs of the
//                        comma-separated list one after the other, their records in file order, into the one output.
//   the index            python/utils/Fasta.py:11-27          FASTA.fai: the lines of exactly five blank-separated fields, fields 1 ... 4
//                        integers (length, offset, bases per line, bytes per line); a later line of one name replaces the earlier one.
//   header: ## lines     python/utils/VCFFile.py:99-113       read up to the column line.  A `##` line with `fileformat` in it sets the
//                        version: it must hold `VCF` or `vcf`; `v3` gives 3, else `v4` or `VCF4` gives 4, else "Cannot determine VCF version".
//   ##INFO=              python/utils/VCFFile.py:115-169      exactly two `"` or "Incomplete description: LINE".  Version 3: the text in
//                        front of the first `"` split on commas is id, number (`.` or an integer), type; an id seen before is "VCF file
//                        already has info-id ID".  Version 4: `<...>` around ("Incorrect description"), split on commas, fields 0 ... 3 are
//                        KEY=value with KEY (blanks removed, upper-cased) ID, NUMBER, TYPE, DESCRIPTION, else "Could not find KEY in: LINE".
//   ##FILTER=            python/utils/VCFFile.py:170-206      the same with id alone (3) and ID, DESCRIPTION in fields 0 and 1 (4).
//   ##FORMAT=            python/utils/VCFFile.py:210-257      as ##INFO=.
//                        A description line in front of the fileformat line reads a version that is not there yet: the script dies.
//   header: column line  python/utils/VCFFile.py:267-284      the first line `#C...`; any other line that is no `##` line is passed over,
//                        an empty one (the end of the file too) kills the script.  Every `#` is removed and the labels are the words
//                        between blanks; a label's column is its last occurrence.  Without an INFO description the warning of
//                        python/utils/VCFFile.py:268-269 goes to stderr.  CHROM POS ID REF ALT QUAL must be there ("Could not find
//                        column X in header of VCF file!"); minLen is the LARGEST COLUMN INDEX, one less than the number of columns.
//   data lines           python/utils/VCFFile.py:287-347      split on tabs only.  An empty line, or one with fewer than minLen fields
//                        ("Cannot parse this line:" and the line on stderr), ENDS THAT FILE'S CONVERSION: both come back as {} and the
//                        loop of python/convertVCFToDindel.py:21-25 breaks on {}.  A line of exactly minLen fields — one short of the last
//                        column — passes that test and kills the script at the missing field; so does a header without INFO or FILTER
//                        column, and a file without fileformat line at its first full data line (python/utils/VCFFile.py:333).  Sample
//                        columns are carried and not looked at.
//   .gz                  python/utils/VCFFile.py:95-98        a name ending in .gz is inflated (every member of the file, so bgzip's output
//                        too; zlib, which the host library links already) and gives the bytes the plain file gives.
//   a record             python/convertVCFToDindel.py:27-42   POS is an integer (else the script dies); the FASTA's letters at POS are
//                        compared with REF first — "REFSEQ inconsistency" on stderr, the line is still written —; the record is used when
//                        QUAL is `.` or float(QUAL) >= minQual (a QUAL that is no number kills the script; the boundary is kept); every
//                        ALT of the comma list on its own; `<DEL>` and an ALT as long as REF are passed over; every other one goes
//                        through Variant4 and writes "%s %d %s\n" % (CHROM, POS + offset - 1, str).
//   the FASTA's letters  python/utils/Fasta.py:34-51          an unknown target prints `KeyError:  NAME` on stdout and raises "KeyError".
//                        Otherwise seek to offset + (POS-1) div blen * llen + (POS-1) mod blen (Python 2's floor division and modulo)
//                        and read len(REF) characters, not counting '\n'; nothing is upper-cased; behind the end of the file every read
//                        gives the empty string and still counts, so the letters come out short.
//   Variant4             python/utils/Variant.py:31-104       see variant4 below.
//   the tool             python/convertVCFToDindel.py:50-76   the three "Please specify" messages with exit code 1, --minQual (default 1).
//
// Where the script dies the functions here throw std::string: a NameError's own text, any other Python exception as `Type: text` with
// Python 2's words.  What is left in the output file after a failure is not part of the contract.
#ifndef DINDEL_VCF_CANDIDATES_HPP
#define DINDEL_VCF_CANDIDATES_HPP
#include <iosfwd>
#include <string>

namespace dindel {

// Variant4 of python/utils/Variant.py:31-104 for alleles of unequal length (the only ones the conversion hands it,
// python/convertVCFToDindel.py:39): type "ins" (ALT longer) or "del"; the shorter allele is the one whose numrb bases "need to be
// identified" in the longer one.  left_match / right_match: the longest common prefix / suffix, at most numrb
// (python/utils/Variant.py:79-86).  left_match == 0 or left_match + right_match < numrb throws "Don't think this is a proper VCF4
// insertion" (python/utils/Variant.py:88-89).  left_end = 1 unless numrb - 1 > right_match, then left_match
// (python/utils/Variant.py:92-95); seq = longer[left_end : len(longer) - (numrb - left_end)] (python/utils/Variant.py:97-100; a
// right_start of 0 takes the slice to the end); offset = left_end; str = "+seq" / "-seq".
struct Variant4 {
    std::string type, seq, str;
    int offset;
    Variant4() : offset(0) {}
};
Variant4 variant4(const std::string &ref, const std::string &alt);

struct VcfConvertOptions {
    std::string inputFiles, outputFile, refFile;      // -i F[,G...], -o, -r
    double minQual;                                   // --minQual (1)
    bool haveRegion; std::string tid; int start, end; // --tid NAME --region A-B (this tool's own): only lines of NAME with start <= position < end
    VcfConvertOptions() : minQual(1.0), haveRegion(false), start(0), end(0) {}
};
// convert of python/convertVCFToDindel.py:9-47; returns the number of lines written.  What the script writes to stderr goes to `err`,
// its one line on stdout to `out`.  Throws std::string where the script dies.
long convertVcfToCandidates(const VcfConvertOptions &opt, std::ostream &err, std::ostream &out);

// float(s) of Python for a string (QUAL, --minQual): blanks around a decimal number, inf / infinity / nan in any case; no hexadecimal.
// Throws "ValueError: could not convert string to float: S".
double pythonFloat(const std::string &s);

// the tool (host/vcf_candidates_main.cpp; host/dindel_vcf2candidates.cpp is this call)
int vcfCandidatesMain(int argc, char **argv);

} // namespace dindel
#endif
