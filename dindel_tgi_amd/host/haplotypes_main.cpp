// haplotypes_main.cpp — the tool dindel_haplotypes: BAM + FASTA + window file -> the W / R / H records dindel_hapalign reads
// (host/window_io.hpp).  Per window: getReads (get_reads.cpp, the selection dindel_gpu makes), the reads' CIGARs, flags and raw letters
// from their records, then getHaplotypesBatch (host/haplotypes.cpp) for every --batchWindows windows.
// Known difference from the reference, kept by this tool: the read buffer is emptied behind a window whose getReads threw, not behind one
// whose haplotype construction threw (it learns that a batch later), and such a window's message does not travel through the W / R / H
// file.  dindel_gpu --ref builds the haplotypes inside the window loop and has neither difference.
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <set>
#include <sstream>
#include "get_reads.hpp"
#include "glf_to_vcf.hpp"
#include "haplotypes.hpp"

namespace dindel {

namespace {

const char *kUsage =
    "usage: dindel_haplotypes --bamFile F | --bamFiles LIST --ref FASTA --varFile WINDOWS --outputFile OUT [options]\n"
    "  candidate haplotypes of every window, from the empirical haplotype distribution of its reads and the window's candidate variants:\n"
    "  W <index> <leftPos> <rightPos> / R <reference sequence of the block> / H <sequence> records for dindel_hapalign --hapFile\n"
    "  read selection (as dindel_gpu): [--varFileIsOneBased] [--maxRead N] [--maxReadLength N] [--minReadOverlap N] [--mapQualThreshold X]\n"
    "                                  [--filterReadAux STR] [--libFile F]\n"
    "  --maxHap N             combinations the blocks are thinned to (default 8)\n"
    "  --skipMaxHap N         a window with more haplotypes is skipped (default 200)\n"
    "  --maxHapReadProd N     ... or with more haplotypes x reads (default 10000000)\n"
    "  --changeINStoN         candidate insertions enter the haplotypes as N\n"
    "  --batchWindows N       windows per device launch (default 1024)\n"
    "  --device D             GPU ordinal (default 0)\n"
    "  --hostDistribution     compute the block tables on the host instead of the device\n"
    "  --quiet                no progress on stderr\n"
    "  --help                 this text\n";

struct Pending { int index; std::string tid; uint32_t pos; };

std::string upper(std::string s)
{
    for (size_t i = 0; i < s.size(); i++) s[i] = char(toupper((unsigned char)s[i]));
    return s;
}

} // namespace

std::string refPiece(IndexedFasta &fa, const std::string &tid, long first1, long last1)
{
    const long len = fa.length(tid);
    if (len < 0) throw std::string("Cannot find sequence ").append(tid).append(" in the reference");
    last1 = std::min(last1, len);
    if (first1 > last1) return std::string();
    return fa.get(tid, first1, int(last1 - first1 + 1));
}

void addWindowReads(HapBatchData &data, const std::vector<Read> &reads)
{
    std::vector<uint32_t> cigar;
    std::string letters;
    for (size_t r = 0; r < reads.size(); r++) {
        if (!reads[r].record) throw std::string("a selected read came without its record");
        const RawBamView v(reads[r].record->data(), reads[r].record->size());
        cigar.resize(v.nCigar());
        for (uint32_t k = 0; k < v.nCigar(); k++) cigar[k] = v.cigar(k);
        letters.resize(size_t(std::max(v.lSeq(), 0)));
        for (int32_t x = 0; x < v.lSeq(); x++) letters[size_t(x)] = v.base(x);
        data.addRead(v.pos(), int32_t(v.flag()), cigar.data(), cigar.size(), letters);
    }
}

int haplotypesMain(int argc, char **argv)
{
    std::map<std::string, std::string> val;
    std::set<std::string> flag;
    static const char *const withValue[] = {"bamFile", "bamFiles", "ref", "varFile", "outputFile", "maxRead", "maxReadLength", "minReadOverlap", "mapQualThreshold",
                                            "filterReadAux", "libFile", "maxHap", "skipMaxHap", "maxHapReadProd", "batchWindows", "device"};
    static const char *const withoutValue[] = {"varFileIsOneBased", "changeINStoN", "hostDistribution", "quiet"};
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--help" || a == "-h") { std::cout << kUsage; return 0; }
        const std::string name = a.size() > 2 && a[0] == '-' && a[1] == '-' ? a.substr(2) : std::string();
        bool known = false;
        for (size_t k = 0; k < sizeof(withValue) / sizeof(*withValue) && !known; k++)
            if (name == withValue[k] && i + 1 < argc) { val[name] = argv[++i]; known = true; }
        for (size_t k = 0; k < sizeof(withoutValue) / sizeof(*withoutValue) && !known; k++)
            if (name == withoutValue[k]) { flag.insert(name); known = true; }
        if (!known) { std::cerr << "dindel_haplotypes: unknown or incomplete option " << a << "\n" << kUsage; return 2; }
    }
    if (!val.count("bamFile") && !val.count("bamFiles")) { std::cerr << "Error: Specify either --bamFile or --bamFiles." << std::endl; return 1; }
    for (const char *need : {"ref", "varFile", "outputFile"})
        if (!val.count(need)) { std::cerr << "Please specify --" << need << std::endl; return 1; }
    auto num = [&](const char *k, double dflt) { return val.count(k) ? atof(val[k].c_str()) : dflt; };
    HaplotypeOptions opt;
    opt.maxHap = size_t(num("maxHap", 8)); opt.skipMaxHap = size_t(num("skipMaxHap", 200)); opt.maxHapReadProd = num("maxHapReadProd", 10000000.0);
    opt.changeINStoN = flag.count("changeINStoN") != 0; opt.hostDistribution = flag.count("hostDistribution") != 0;
    opt.device = int(num("device", 0));
    const int batchWindows = int(num("batchWindows", 1024));
    const bool quiet = flag.count("quiet") != 0, oneBased = flag.count("varFileIsOneBased") != 0;
    if (batchWindows < 1) { std::cerr << "dindel_haplotypes: --batchWindows must be at least 1" << std::endl; return 2; }
    if (num("maxHap", 8) < 1 || num("skipMaxHap", 200) < 1) { std::cerr << "dindel_haplotypes: --maxHap and --skipMaxHap must be at least 1" << std::endl; return 2; }
    ReadSelectionParameters rsp;
    rsp.maxReads = size_t(num("maxRead", double(rsp.maxReads))); rsp.maxReadLength = size_t(num("maxReadLength", double(rsp.maxReadLength)));
    rsp.minReadOverlap = int(num("minReadOverlap", rsp.minReadOverlap)); rsp.mapQualThreshold = num("mapQualThreshold", rsp.mapQualThreshold);
    rsp.quiet = true; rsp.keepRecords = true;                  // the CIGAR, the flag and the raw letters come from the record
    if (val.count("filterReadAux")) rsp.filterReadAux = val["filterReadAux"];
    if (val.count("libFile")) rsp.mapUnmappedReads = true;      // as in dindel_gpu (DInDel.cpp:4268-4272)

    try {
        LibraryCollection libraries;
        if (rsp.mapUnmappedReads) libraries.addFromFile(val["libFile"]);
        std::vector<std::string> bamPaths;
        if (val.count("bamFile")) bamPaths.push_back(val["bamFile"]);
        else {
            std::ifstream list(val["bamFiles"].c_str());
            if (!list.is_open()) { std::cout << "Cannot open file with BAM files:  " << val["bamFiles"] << std::endl; throw std::string("File open error."); }
            std::string line;
            while (std::getline(list, line)) { std::istringstream is(line); std::string f; if (is >> f) bamPaths.push_back(f); }
            if (bamPaths.empty()) throw std::string("No BAM file in ").append(val["bamFiles"]);
        }
        BamFileSet bams(bamPaths);
        ReadFetcher fetcher(bams.pointers(), libraries, rsp);
        IndexedFasta fa(val["ref"]);
        VariantFile vf(val["varFile"]);
        std::ofstream out(val["outputFile"].c_str());
        if (!out) throw std::string("Cannot open output file ").append(val["outputFile"]);

        size_t nWindows = 0, nWritten = 0, nHaps = 0, stats[2] = {0, 0};
        HapBatchData data;
        std::vector<WindowCandidates> wins;
        std::vector<Pending> pending;
        auto flush = [&]() {
            getHaplotypesBatch(data, wins, opt, stats);
            for (size_t k = 0; k < wins.size(); k++) {
                const WindowCandidates &w = wins[k];
                if (!w.message.empty()) { std::cerr << "tid: " << pending[k].tid << " pos: " << pending[k].pos << " " << w.message << std::endl; continue; }
                out << "W " << pending[k].index << " " << w.leftPos << " " << w.rightPos << "\n";
                out << "R " << upper(refPiece(fa, pending[k].tid, long(w.leftPos) + 1, long(w.rightPos) + 1)) << "\n";
                for (size_t h = 0; h < w.haps.size(); h++) out << "H " << w.haps[h] << "\n";
                nWritten++; nHaps += w.haps.size();
            }
            data = HapBatchData(); wins.clear(); pending.clear();
            if (!quiet) std::cerr << "dindel_haplotypes: " << nWindows << " windows" << std::endl;
        };

        int index = 0;
        std::string oldTid("-1");
        uint32_t oldLeftPos = 0;
        std::vector<Read> reads;
        while (!vf.eof()) {
            AlignedCandidates cand = vf.getLineVector(oneBased);
            if (cand.variants.size() == 0) continue;
            if (cand.tid != oldTid) { oldTid = cand.tid; oldLeftPos = 0; fetcher.newChromosome(); }
            if (uint32_t(cand.leftPos) < oldLeftPos) {
                std::cerr << "leftPos: " << uint32_t(cand.leftPos) << " oldLeftPos: " << oldLeftPos << std::endl;
                std::cerr << "Candidate variant files must be sorted on left position of window!" << std::endl;
                if (!wins.empty()) flush();
                return 1;
            }
            oldLeftPos = uint32_t(cand.leftPos);
            ++index; nWindows++;
            bool skipped = false;
            try { fetcher.getReads(cand.tid, uint32_t(cand.leftPos), uint32_t(cand.rightPos), reads); }
            catch (std::string &s) { std::cerr << "tid: " << cand.tid << " pos: " << cand.centerPos << " " << s << std::endl; skipped = true; }
            fetcher.windowDone(skipped, uint32_t(cand.leftPos));
            if (skipped) continue;
            // DInDel.cpp:1530-1532
            const uint32_t rs = cand.leftPos > rsp.minReadOverlap ? uint32_t(cand.leftPos - rsp.minReadOverlap) : 0u, re = uint32_t(cand.rightPos + rsp.minReadOverlap);
            data.addWindow(int32_t(rs), refPiece(fa, cand.tid, long(rs) + 1, long(re) + 1));
            addWindowReads(data, reads);
            WindowCandidates w;
            w.leftPos = uint32_t(cand.leftPos); w.rightPos = uint32_t(cand.rightPos); w.variants = cand.variants; w.nReads = reads.size();
            wins.push_back(w);
            const Pending p = {index, cand.tid, uint32_t(cand.centerPos)};
            pending.push_back(p);
            if (int(wins.size()) >= batchWindows) flush();
        }
        if (!wins.empty()) flush();
        out.flush();
        if (!out) throw std::string("Cannot write output file ").append(val["outputFile"]);
        if (!quiet)
            std::cerr << "dindel_haplotypes: " << nWindows << " windows, " << nWritten << " written with " << nHaps << " haplotypes; block tables: " << stats[0]
                      << (opt.hostDistribution ? " on the host" : " on the device") << ", " << stats[1] << " through the sequential path" << std::endl;
    } catch (std::string &s) {
        std::cerr << "dindel_haplotypes: " << s << std::endl;
        return 1;
    } catch (ReadFetcher::FatalError &e) {
        std::cerr << "dindel_haplotypes: " << e.message << std::endl;
        return e.exitCode;
    }
    return 0;
}

} // namespace dindel
