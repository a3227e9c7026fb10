// discover.cpp — see discover.hpp.
#include "discover.hpp"
#include <fstream>
#include <iostream>
#include <sstream>

namespace dindel {

std::vector<std::string> readBamList(const std::string &listFile)
{
    std::ifstream list(listFile.c_str());
    if (!list.is_open()) throw std::string("Cannot open file with BAM files.");
    std::vector<std::string> bams;
    std::string line;
    while (std::getline(list, line)) {
        std::istringstream is(line);
        std::string fname;
        is >> fname;
        if (!fname.empty()) bams.push_back(fname);
    }
    return bams;
}

// step a.: the BAM pass
static void candidatesOfTheSample(const DiscoverOptions &opt, CandidateStats &stats)
{
    if (opt.bamFiles.empty()) throw std::string("No BAM file to discover candidates in.");
    if (!opt.haveRegion && opt.bamFiles.size() != 1) throw std::string("Can extract the full set of indels from only BAM file at a time.");
    IndexedFasta fa(opt.refFile);
    if (opt.haveRegion) {
        if (!opt.candidates.quiet)
            std::cout << "Getting indels from CIGARs in mapped reads from region " << opt.tid << ":" << opt.start << "-" << opt.end << std::endl;
        candidatesFromRegion(opt.bamFiles, opt.tid, opt.start, opt.end, opt.variantsFile(), fa, opt.candidates, stats);
    } else {
        if (!opt.candidates.quiet) std::cout << "Reading BAM file: " << opt.bamFiles[0] << std::endl;
        candidatesFromBam(opt.bamFiles[0], opt.outputPrefix, fa, opt.candidates, stats);
    }
}

static std::vector<std::string> linesOf(const std::string &file)
{
    std::ifstream in(file.c_str());
    if (!in.is_open()) throw std::string("Cannot open file ").append(file);
    std::vector<std::string> lines;
    std::string line;
    while (std::getline(in, line)) lines.push_back(line);
    return lines;
}

// steps c., d. and e.: the known sites, realigned, behind what is kept of the sample's own candidates
static void candidatesWithKnownSites(const DiscoverOptions &opt, CandidateStats &stats)
{
    std::ostringstream silent;
    const bool quiet = opt.candidates.quiet;
    VcfConvertOptions c;
    c.inputFiles = opt.candidateVCF; c.outputFile = opt.vcfVariantsFile(); c.refFile = opt.refFile; c.minQual = opt.minQual;
    c.haveRegion = opt.haveRegion; c.tid = opt.tid; c.start = opt.start; c.end = opt.end;
    convertVcfToCandidates(c, quiet ? static_cast<std::ostream &>(silent) : std::cerr, quiet ? static_cast<std::ostream &>(silent) : std::cout);
    {
        IndexedFasta fa(opt.refFile);
        realignCandidateFile(opt.vcfVariantsFile(), false, opt.vcfRealignedFile(), fa, opt.candidates, stats);
    }
    std::vector<std::string> lines;
    if (!opt.vcfCandidatesOnly) {
        lines = linesOf(opt.variantsFile());
        if (opt.filter) lines = selectCandidates(lines, opt.minCount, opt.maxCount, quiet ? static_cast<std::ostream &>(silent) : std::cerr);
    }
    const std::vector<std::string> known = linesOf(opt.vcfRealignedFile());
    lines.insert(lines.end(), known.begin(), known.end());
    std::ofstream out(opt.candidatesFile().c_str());
    if (!out.is_open()) throw std::string("Cannot open file ").append(opt.candidatesFile()).append(" for writing.");
    for (size_t l = 0; l < lines.size(); l++) out << lines[l] << "\n";
}

long discoverWindows(const DiscoverOptions &opt, CandidateStats &stats)
{
    const bool known = !opt.candidateVCF.empty();
    if (opt.vcfCandidatesOnly && !known) throw std::string("--vcfCandidatesOnly needs --candidateVCF.");
    if (opt.vcfCandidatesOnly && opt.filter) throw std::string("--minCount / --maxCount filter the sample's own candidates: with --vcfCandidatesOnly there are none.");
    if (!opt.vcfCandidatesOnly) candidatesOfTheSample(opt, stats);
    if (known) candidatesWithKnownSites(opt, stats);
    WindowOptions w;
    w.inputVarFile = known ? opt.candidatesFile() : opt.variantsFile();
    w.oneFile = opt.windowsFile();
    w.minDist = opt.minDist;
    if (!known) { w.filter = opt.filter; w.minCount = opt.minCount; w.maxCount = opt.maxCount; }
    w.quiet = opt.candidates.quiet;
    return writeWindows(w, std::cerr);
}

} // namespace dindel
