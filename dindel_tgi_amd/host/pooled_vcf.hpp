// pooled_vcf.hpp — the end of the pooled workflow: the `singlevariant` lines of `dindel_gpu --doPooled` (PREFIX.glf.txt) -> a VCF of
// calls, and the per-pool genotype likelihoods of the called sites.  Restates the reference's Python-2 scripts
// python/mergeOutputPooled.py (processPooledGLFFiles, getPercentiles) and python/makeGenotypeLikelihoodFilePooled.py (makeGLF) with the parts
// of FileUtils.py, Variant.py, Fasta.py and AnalyzeSequence.py they run, rule for rule; plain C++, no GPU: text, integer and a little double
// work per line.  Files are taken as bytes, as Python 2 takes them; a name ending in .gz is inflated first and gives the plain file's bytes.
//
// processPooledGLFFiles
//   list file            python/mergeOutputPooled.py:209-239  every blank-separated word of every line is a path.  A missing file and an
//                        empty one get their WARNING on stderr and are left out.  The first header seen, split on blanks, is the header; a
//                        file whose first line differs gets "Inconsistent header in GLF file ..." and is left out.
//   columns              python/mergeOutputPooled.py:251-273  realigned_position, nref_all, num_reads, num_cover_forward, num_cover_reverse,
//                        var_coverage_forward, var_coverage_reverse, post_prob_variant, tid, indidx, analysis_type: one missing (no file
//                        left too) is "GLF files are corrupt. Could not find all required columns.".  est_freq is looked up at the first
//                        completed group (python/mergeOutputPooled.py:357): a ValueError there.
//   reading              python/mergeOutputPooled.py:282-379, FileUtils.py:123-137  lines in groups of numBamFiles; a line is right-stripped
//                        and split on single blanks.  An empty line or the end of the file ends that file and drops a group begun.  A wrong
//                        number of fields writes "Line in file ... does not have the correct number of labels" and kills the script (None is
//                        subscripted: a TypeError).  realigned_position NA, or analysis_type other than singlevariant, ends the group THERE:
//                        its remaining lines are not consumed, the next group starts at the next line.  indidx >= numBamFiles and a position
//                        differing inside a group are the two NameErrors; indidx != place in the group only writes "Error reading this
//                        variant".  NFS / NRS sum num_cover_forward / _reverse over the group, NF / NR are var_coverage_* of the group's
//                        FIRST line, DP sums num_reads, NS counts lines with num_reads > 0; QUAL and AF are post_prob_variant and est_freq
//                        of the group's LAST line.  Every completed group counts into the depth histogram; a group with prob > 0.20 is
//                        recorded under (tid, pos, variant), a later one replacing an earlier one.
//   getPercentiles       python/mergeOutputPooled.py:8-32     as written: at most one percentile advances per distinct depth, so one depth
//                        value k alone gives the range [k, 0] and every variant is `ocr`.
//   filters              python/mergeOutputPooled.py:386-425  in this order: q<filterQual> (prob < 1 - 10^(-filterQual/10)), fr0 (with
//                        --filterFR: NF or NR below 1), ocr, s50 (NS < numSamples div 2, Python 2's integer division), hp<maxHPLen>,
//                        mf (AF < 1/(10 numSamples)).
//   header, order        python/mergeOutputPooled.py:428-465  the fr0 line only with --filterFR, the ocr line with the measured range.
//                        Chromosomes 1 ... 22, X, Y, then the others.  A chromosome without a PASS variant writes NO line at all.
//   closeness            python/mergeOutputPooled.py:468-531  over the positions with a PASS variant, minDist 10.  The best position of a
//                        merged site has the largest per-position maximum QUAL.  At every other position of the site a variant whose filter
//                        string is non-empty gets `;tc10`; a PASS variant STAYS PASS (python/mergeOutputPooled.py:529 compares, it does not
//                        assign).
//   a line               python/mergeOutputPooled.py:537-574  positions ascend; qual = -trunc(10 log10(max(1 - QUAL, 1e-10))); REF and ALT
//                        from the FASTA at (chr, pos, 1 + deletion length); INFO AF NS DP HP NF NR NFS NRS with AF as Python 2's str(float).
//                        A `X=>Y` variant dies at python/mergeOutputPooled.py:563 (IndexError: refseq has one letter).
// Knowing deviations, all where the script's order is a Python-2 hash table's: the chromosomes other than 1 ... 22, X, Y follow in ascending
// byte order (host/glf_to_vcf.cpp's rule); several variants of one position are written in ascending byte order of the variant string; on a
// tie of QUAL between the positions of a merged site the LOWEST position wins (the order Python 3 gives).
//
// makeGLF
//   getCalls             python/makeGenotypeLikelihoodFilePooled.py:10-46   the VCF as a tab-separated table whose header is the first
//                        `#X` line (FileUtils.py:43-50; a file without one makes the script spin: an IOError here).  A record is kept when
//                        FILTER is PASS, or q20 with float(QUAL) >= 10.  A comma in ALT: "Cannot deal with these entries".  The key is
//                        (CHROM, POS + offset - 1, str) of Variant4(REF, ALT), Variant.py:31-104; twice: "Multiple same variants?".
//   loadGLFFiles         python/makeGenotypeLikelihoodFilePooled.py:110-141 the first word of each line of the list; a missing file gets
//                        "File ... does not exist" and is left out; the files are ordered by their first realigned_position that is not NA
//                        (the position alone is the key: a second file with the same one raises "Huh?").
//   the walk             python/makeGenotypeLikelihoodFilePooled.py:49-107, :175-206  consecutive lines are grouped by
//                        index.realigned_position.nref_all.  Per group, in this order: nref_all NA -> na-error; not among the calls ->
//                        notcalled; group length != number of BAM names -> "Skipping index ..." on stderr; else one line
//                        `tid pos nref_all L00 L01 L11 NAME[indidx]` per line of the group, `glf` split on `;` and `:` — a missing 0/0, 0/1
//                        or 1/1 is a KeyError, which is what a `dip.map` line of a called site gives.
//
// Where a script dies the functions throw std::string: a NameError's own text, any other exception as `Type: text` in Python 2's words.  What
// is left in the output file after a failure is not part of the contract.
#ifndef DINDEL_POOLED_VCF_HPP
#define DINDEL_POOLED_VCF_HPP
#include <iosfwd>
#include <map>
#include <string>
#include <vector>
#include "vcf_candidates.hpp"

namespace dindel {

// getPercentiles (python/mergeOutputPooled.py:8-32): hist is depth -> count
std::vector<long> getPercentiles(const std::map<long, long> &hist, const std::vector<int> &pctiles);

// Python 2's str(x) of a float: %.12g, and `.0` behind it when the text has neither `.`, `e`, `inf` nor `nan`
std::string pythonStrFloat(double x);

struct PooledVcfOptions {
    std::string outputFile, refFile;         // -o, -r
    int numSamples, numBamFiles, maxHPLen, filterQual;   // --numSamples, --numBamFiles (1), --maxHPLen (10), --filterQual (20)
    bool filterFR;                           // --filterFR
    PooledVcfOptions() : numSamples(1), numBamFiles(1), maxHPLen(10), filterQual(20), filterFR(false) {}
};
// processPooledGLFFiles (python/mergeOutputPooled.py:202-575) behind its list file: the words of that file, in order.  What the script writes
// on stderr goes to `err`, what it prints to `out`.  Throws std::string where the script dies.
void pooledGlfToVcf(const std::vector<std::string> &glfFiles, const PooledVcfOptions &opt, std::ostream &err, std::ostream &out);
// ... with the list file (-i)
void processPooledGLFFiles(const std::string &glfFilesFile, const PooledVcfOptions &opt, std::ostream &err, std::ostream &out);

// Variant4 of Variant.py:31-104 for any pair of alleles: unequal lengths are variant4 (host/vcf_candidates.hpp); equal lengths are
// Variant.py:37-62: one mismatch is the "snp" `X=>Y` with the mismatch's index as offset, none dies at the first use of the offset that was
// never set (an AttributeError), more is "MultiSNP".
Variant4 variant4AnyLength(const std::string &ref, const std::string &alt);

// makeGLF (python/makeGenotypeLikelihoodFilePooled.py:146-213) behind its two list files: the .glf.txt files and the BAM names, in order
void pooledCallsToGlf(const std::vector<std::string> &glfFiles, const std::string &callFile, const std::string &outputFile,
                      const std::vector<std::string> &bamNames, std::ostream &err, std::ostream &out);
// ... with the list files (-g, -b): the first word of each line
void makeGLF(const std::string &inputGLFFiles, const std::string &outputFile, const std::string &callFile, const std::string &bamfilesFile,
             std::ostream &err, std::ostream &out);

// the tools (host/dindel_pooled2vcf.cpp and host/dindel_pooled2glf.cpp are these calls)
int pooledVcfMain(int argc, char **argv);
int pooledGlfMain(int argc, char **argv);

} // namespace dindel
#endif
