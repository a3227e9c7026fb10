// vcf_candidates_main.cpp — the tool dindel_vcf2candidates: the options, messages and exit codes of the reference's
// python/convertVCFToDindel.py:50-88, and --tid / --region of its own (a line filter, parsed by candidates.hpp's parseRegion).
#include <iostream>
#include <sstream>
#include "candidates.hpp"
#include "vcf_candidates.hpp"

namespace dindel {

namespace {
const char *kUsage =
    "usage: dindel_vcf2candidates -i VCF[,VCF...] -o OUT -r FASTA [options]        (the reference's python/convertVCFToDindel.py)\n"
    "  -i, --inputFile F[,G...]    VCF file(s) of known indels, plain or .gz; several are read one after the other into the one output\n"
    "  -o, --outputFile OUT        output file with Dindel-style variants: `tid pos variant` lines, zero-based, for\n"
    "                              dindel_candidates --analysis realignCandidates\n"
    "  -r, --refFile FASTA         reference sequence, with FASTA.fai\n"
    "  --minQual X                 use the records with QUAL `.` or QUAL >= X (default 1)\n"
    "  --tid NAME --region A-B     write only the lines of target NAME whose position lies in [A, B)\n"
    "  --quiet                     none of the script's notes on stderr (REFSEQ inconsistency, lines that cannot be parsed, the INFO warning)\n"
    "  -h, --help                  this text\n";
}

int vcfCandidatesMain(int argc, char **argv)
{
    VcfConvertOptions opt;
    std::string minQual, region;
    bool quiet = false, haveTid = false, haveRegion = false;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        const char *v = i + 1 < argc ? argv[i + 1] : NULL;
        if (a == "-h" || a == "--help") { std::cout << kUsage; return 0; }
        else if (a == "--quiet") quiet = true;
        else if ((a == "-i" || a == "--inputFile") && v) { opt.inputFiles = v; i++; }
        else if ((a == "-o" || a == "--outputFile") && v) { opt.outputFile = v; i++; }
        else if ((a == "-r" || a == "--refFile") && v) { opt.refFile = v; i++; }
        else if (a == "--minQual" && v) { minQual = v; i++; }
        else if (a == "--tid" && v) { opt.tid = v; haveTid = true; i++; }
        else if (a == "--region" && v) { region = v; haveRegion = true; i++; }
        else { std::cerr << "dindel_vcf2candidates: error: no such option, or no value for it: " << a << "\n"; return 2; }
    }
    if (opt.inputFiles.empty()) { std::cerr << "Please specify --inputFile\n"; return 1; }                  // python/convertVCFToDindel.py:60-68
    if (opt.outputFile.empty()) { std::cerr << "Please specify --outputFile\n"; return 1; }
    if (opt.refFile.empty()) { std::cerr << "Please specify --refFile\n"; return 1; }
    if (haveTid != haveRegion) { std::cerr << "--tid and --region go together: --tid NAME --region A-B\n"; return 1; }
    std::ostringstream silent;
    try {
        if (!minQual.empty()) opt.minQual = pythonFloat(minQual);                                           // python/convertVCFToDindel.py:73
        if (haveRegion) { opt.haveRegion = true; parseRegion(region, opt.start, opt.end); }
        convertVcfToCandidates(opt, quiet ? static_cast<std::ostream &>(silent) : std::cerr, quiet ? static_cast<std::ostream &>(silent) : std::cout);
    } catch (const std::string &s) {
        std::cerr << "An error occurred!\n" << s << "\n";                                                   // python/convertVCFToDindel.py:84-87
        return 1;
    }
    return 0;
}

} // namespace dindel
