// discover.hpp — the discovery stage of dindel_gpu --discover: steps 1 and 3 of the workflow in front of the window loop.
//   a. candidatesFromBam / candidatesFromRegion (candidates.hpp; reference GetCandidates.cpp:387-486, GetCandidates.cpp:50-62) write
//      PREFIX.variants.txt and, for a whole-file run, PREFIX.libraries.txt: the code, launches and bytes of
//      `dindel_candidates --analysis getCIGARindels`;
//   b. writeWindows (windows.hpp; python/makeWindows.py:129-207) makes PREFIX.windows.txt from it, every line in the one file.
// With a VCF of known sites (--candidateVCF) the stage is the tools run one after the other:
//   a. as above, unless vcfCandidatesOnly;
//   c. convertVcfToCandidates (vcf_candidates.hpp; python/convertVCFToDindel.py:9-47) writes PREFIX.vcf.variants.txt — what
//      `dindel_vcf2candidates -i ... -o PREFIX.vcf.variants.txt -r REF [--minQual X]` writes, with --tid / --region in a region run;
//   d. realignCandidateFile (candidates.hpp; reference GetCandidates.cpp:260-303) writes PREFIX.vcf.realigned.variants.txt — what
//      `dindel_candidates --analysis realignCandidates --varFile PREFIX.vcf.variants.txt --outputFile PREFIX.vcf.realigned` writes, with
//      the same CandidateOptions (and so the same AlignHook) as a.;
//   e. PREFIX.candidates.txt: the lines of PREFIX.variants.txt that --minCount / --maxCount keep (what `dindel_windows --selectedFile`
//      writes; all of the file without a filter), then every line of d.'s file: known sites are never filtered;
//   b. writeWindows on PREFIX.candidates.txt, without a filter.
// The stage is a barrier in front of the loop: a window is a cluster of neighbouring candidates, and which candidates are neighbours is
// known only when the target's whole table has been realigned and written.
#ifndef DINDEL_DISCOVER_HPP
#define DINDEL_DISCOVER_HPP
#include <string>
#include <vector>
#include "candidates.hpp"
#include "vcf_candidates.hpp"
#include "windows.hpp"

namespace dindel {

struct DiscoverOptions {
    std::vector<std::string> bamFiles;                // one file: a whole-file run unless a region is given; several: region runs only
    bool haveRegion; std::string tid; int start, end; // --tid NAME --region A-B
    std::string refFile, outputPrefix;
    CandidateOptions candidates;                      // device, --batchCandidates, --eventsCap, --hostConvert, quiet, and the AlignHook
    long minDist;                                     // --minDist (20)
    bool filter; long minCount, maxCount;             // --minCount / --maxCount
    std::string candidateVCF;                         // --candidateVCF F[,G...]: known sites beside the BAM's own candidates (empty: none)
    double minQual;                                   // --minQual (1)
    bool vcfCandidatesOnly;                           // --vcfCandidatesOnly: no BAM pass; the filter options are an error
    DiscoverOptions() : haveRegion(false), start(0), end(0), minDist(20), filter(false), minCount(2), maxCount(10000000), minQual(1.0), vcfCandidatesOnly(false) {}
    std::string variantsFile() const { return outputPrefix + ".variants.txt"; }
    std::string librariesFile() const { return outputPrefix + ".libraries.txt"; }       // (whole-file runs only)
    std::string windowsFile() const { return outputPrefix + ".windows.txt"; }
    std::string vcfVariantsFile() const { return outputPrefix + ".vcf.variants.txt"; }  // (the three files of a --candidateVCF run)
    std::string vcfRealignedPrefix() const { return outputPrefix + ".vcf.realigned"; }
    std::string vcfRealignedFile() const { return vcfRealignedPrefix() + ".variants.txt"; }
    std::string candidatesFile() const { return outputPrefix + ".candidates.txt"; }
};

// Runs a. and b., or with candidateVCF a., c., d., e. and b.; returns the number of window lines written to windowsFile().  Throws std::string.
long discoverWindows(const DiscoverOptions &opt, CandidateStats &stats);

// `--bamFiles LIST`: one path per line, the first word of the line (reference DInDel.cpp:64-88).  Throws std::string.
std::vector<std::string> readBamList(const std::string &listFile);

} // namespace dindel
#endif
