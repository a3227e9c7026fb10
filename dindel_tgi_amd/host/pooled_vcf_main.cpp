// pooled_vcf_main.cpp — the tools dindel_pooled2vcf and dindel_pooled2glf: the options, messages and exit codes of the reference's
// python/mergeOutputPooled.py:577-620 and python/makeGenotypeLikelihoodFilePooled.py:227-245.
#include <iostream>
#include <sstream>
#include "pooled_vcf.hpp"
#include "python_text.hpp"

namespace dindel {

namespace {
const char *kVcfUsage =
    "usage: dindel_pooled2vcf -i LIST -o OUT.vcf -r FASTA --numSamples N [options]        (the reference's python/mergeOutputPooled.py)\n"
    "  -i, --inputFiles LIST       file that contains the list of '.glf.txt' files of dindel_gpu --doPooled that should be merged (plain or .gz)\n"
    "  -o, --outputFile OUT        output VCF file with variant calls\n"
    "  -r, --refFile FASTA         reference sequence, with FASTA.fai\n"
    "  --numSamples N              number of samples\n"
    "  --numBamFiles N             number of BAM files, i.e. of lines per variant (default 1)\n"
    "  --maxHPLen N                maximum length of homopolymer run to call an indel (default 10)\n"
    "  --filterFR                  filter on forward/reverse count of reads (stringent)\n"
    "  --filterQual Q              quality below which variants are filtered (default 20)\n"
    "  --quiet                     none of the script's progress lines on stdout\n"
    "  -h, --help                  this text\n";
const char *kGlfUsage =
    "usage: dindel_pooled2glf -g LIST -c CALLS.vcf -o OUT -b BAMLIST        (the reference's python/makeGenotypeLikelihoodFilePooled.py)\n"
    "  -g, --inputGLFFiles LIST    file with all '.glf.txt' files\n"
    "  -c, --callFile VCF          VCF file with calls (as produced by dindel_pooled2vcf)\n"
    "  -o, --outputFile OUT        output file: `tid pos variant L00 L01 L11 NAME` per called site and pool\n"
    "  -b, --bamFiles BAMLIST      file with the list of BAM files / IDs, in the order of the file given to dindel_gpu --bamFiles\n"
    "  --quiet                     none of the script's progress lines on stdout\n"
    "  -h, --help                  this text\n";
}

int pooledVcfMain(int argc, char **argv)
{
    PooledVcfOptions opt;
    std::string inputFiles, numSamples, numBamFiles = "1", maxHPLen = "10", filterQual = "20";
    bool quiet = false, haveSamples = false;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        const char *v = i + 1 < argc ? argv[i + 1] : NULL;
        if (a == "-h" || a == "--help") { std::cout << kVcfUsage; return 0; }
        else if (a == "--quiet") quiet = true;
        else if (a == "--filterFR") opt.filterFR = true;
        else if ((a == "-i" || a == "--inputFiles") && v) { inputFiles = v; i++; }
        else if ((a == "-o" || a == "--outputFile") && v) { opt.outputFile = v; i++; }
        else if ((a == "-r" || a == "--refFile") && v) { opt.refFile = v; i++; }
        else if (a == "--numSamples" && v) { numSamples = v; haveSamples = true; i++; }
        else if (a == "--numBamFiles" && v) { numBamFiles = v; i++; }
        else if (a == "--maxHPLen" && v) { maxHPLen = v; i++; }
        else if (a == "--filterQual" && v) { filterQual = v; i++; }
        else { std::cerr << "dindel_pooled2vcf: error: no such option, or no value for it: " << a << "\n"; return 2; }
    }
    if (inputFiles.empty()) { std::cerr << "Please specify --inputFiles\n"; return 1; }                    // python/mergeOutputPooled.py:595-607
    if (opt.outputFile.empty()) { std::cerr << "Please specify --outputFile\n"; return 1; }
    if (opt.refFile.empty()) { std::cerr << "Please specify --refFile\n"; return 1; }
    if (!haveSamples) { std::cerr << "Please specify --numSamples option\n"; return 1; }
    std::ostringstream silent;
    try {
        try { opt.maxHPLen = int(pytext::pyInt(maxHPLen)); }                                                // (optparse's type = "int")
        catch (const std::string &) { std::cerr << "dindel_pooled2vcf: error: option --maxHPLen: invalid integer value: '" << maxHPLen << "'\n"; return 2; }
        opt.filterQual = int(pytext::pyInt(filterQual));                                                    // python/mergeOutputPooled.py:609
        opt.numSamples = int(pytext::pyInt(numSamples));
        opt.numBamFiles = int(pytext::pyInt(numBamFiles));
        processPooledGLFFiles(inputFiles, opt, std::cerr, quiet ? static_cast<std::ostream &>(silent) : std::cout);
    } catch (const std::string &s) {
        std::cerr << "An error occurred!\n" << s << "\n";                                                   // python/mergeOutputPooled.py:615-619
        return 1;
    }
    return 0;
}

int pooledGlfMain(int argc, char **argv)
{
    std::string glfs, calls, output, bams;
    bool quiet = false;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        const char *v = i + 1 < argc ? argv[i + 1] : NULL;
        if (a == "-h" || a == "--help") { std::cout << kGlfUsage; return 0; }
        else if (a == "--quiet") quiet = true;
        else if ((a == "-g" || a == "--inputGLFFiles") && v) { glfs = v; i++; }
        else if ((a == "-c" || a == "--callFile") && v) { calls = v; i++; }
        else if ((a == "-o" || a == "--outputFile") && v) { output = v; i++; }
        else if ((a == "-b" || a == "--bamFiles") && v) { bams = v; i++; }
        else { std::cerr << "dindel_pooled2glf: error: no such option, or no value for it: " << a << "\n"; return 2; }
    }
    if (glfs.empty() || calls.empty() || output.empty() || bams.empty()) {                                  // python/makeGenotypeLikelihoodFilePooled.py:236-238
        std::cerr << "Please specify all required options.\n";
        return 1;
    }
    std::ostringstream silent;
    try {
        makeGLF(glfs, output, calls, bams, std::cerr, quiet ? static_cast<std::ostream &>(silent) : std::cout);
    } catch (const std::string &s) {
        std::cerr << s << "\n";                                                                             // (the script's traceback ends with this line)
        return 1;
    }
    return 0;
}

} // namespace dindel
