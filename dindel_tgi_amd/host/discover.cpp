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

long discoverWindows(const DiscoverOptions &opt, CandidateStats &stats)
{
    if (opt.bamFiles.empty()) throw std::string("No BAM file to discover candidates in.");
    if (!opt.haveRegion && opt.bamFiles.size() != 1) throw std::string("Can extract the full set of indels from only BAM file at a time.");
    {
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
    WindowOptions w;
    w.inputVarFile = opt.variantsFile();
    w.oneFile = opt.windowsFile();
    w.minDist = opt.minDist;
    w.filter = opt.filter; w.minCount = opt.minCount; w.maxCount = opt.maxCount;
    w.quiet = opt.candidates.quiet;
    return writeWindows(w, std::cerr);
}

} // namespace dindel
