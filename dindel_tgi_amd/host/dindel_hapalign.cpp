// dindel_hapalign — DetInDel::alignHaplotypes (reference DInDel.cpp:1427-1524) and the end of getHaplotypes (DInDel.cpp:1600-1626) as a
// tool: reads candidate haplotypes with their block's reference sequence (W / R / H records, host/window_io.hpp), aligns every haplotype
// against its reference on the GPU (one launch per batch of windows) and writes the W / H / A / V file dindel_gpu --hapFile reads.
//
//   dindel_hapalign --hapFile IN --outputFile OUT [--device D] [--batchWindows N] [--hostConvert] [--quiet]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>
#include "align_haplotypes.hpp"

using namespace dindel;

static const char *kUsage =
    "usage: dindel_hapalign --hapFile IN --outputFile OUT [--device D] [--batchWindows N] [--hostConvert] [--quiet]\n"
    "  --hapFile IN       W <index> <leftPos> <rightPos> / R <reference sequence of the block> / H <sequence> records;\n"
    "                     A and V records of the input are ignored\n"
    "  --outputFile OUT   W / H / A / V records (no R): the haplotype file of dindel_gpu --hapFile\n"
    "  --device D         GPU ordinal (default 0)\n"
    "  --batchWindows N   windows per device launch (default 1024)\n"
    "  --hostConvert      the variants of every alignment are made on the host from its slice (convertAlignment as a string walk)\n"
    "                     instead of by the variants kernel on the device; the output is the same bytes either way\n"
    "  --quiet            no progress on stderr\n"
    "  --help             this text\n";

static void writeWindow(std::ostream &out, const WindowHaplotypes &w)
{
    out << "W " << w.index << " " << w.leftPos << " " << w.rightPos << "\n";
    for (size_t h = 0; h < w.haps.size(); h++) {
        out << "H " << w.haps[h].seq << "\nA";
        for (size_t b = 0; b < w.haps[h].refHpos.size(); b++) out << " " << w.haps[h].refHpos[b];
        out << "\n";
        for (int s = 0; s < 2; s++) {               // std::map order, indels before SNPs
            const std::map<int, AlignedVariant> &m = s ? w.haps[h].snps : w.haps[h].indels;
            for (std::map<int, AlignedVariant>::const_iterator it = m.begin(); it != m.end(); ++it) {
                const AlignedVariant &v = it->second;
                out << "V " << "IS"[s] << " " << it->first << " " << v.getString() << " " << v.getStartHap() << " " << v.getEndHap() << " " << v.getStartRead()
                    << " " << v.getEndRead() << " " << v.getLeftFlankHap() << " " << v.getRightFlankHap() << " " << v.getLeftFlankRead() << " "
                    << v.getRightFlankRead() << "\n";
            }
        }
    }
}

int main(int argc, char **argv)
{
    std::string hapFile, outFile;
    int device = 0, batchWindows = 1024;
    bool quiet = false, hostConvert = false;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        const bool has = i + 1 < argc;
        if (a == "--help" || a == "-h") { std::cout << kUsage; return 0; }
        else if (a == "--quiet") quiet = true;
        else if (a == "--hostConvert") hostConvert = true;
        else if (a == "--hapFile" && has) hapFile = argv[++i];
        else if (a == "--outputFile" && has) outFile = argv[++i];
        else if (a == "--device" && has) device = atoi(argv[++i]);
        else if (a == "--batchWindows" && has) batchWindows = atoi(argv[++i]);
        else { std::cerr << "dindel_hapalign: unknown or incomplete option " << a << "\n" << kUsage; return 2; }
    }
    if (hapFile.empty() || outFile.empty()) { std::cerr << "dindel_hapalign: --hapFile and --outputFile are required\n" << kUsage; return 2; }
    if (batchWindows < 1) { std::cerr << "dindel_hapalign: --batchWindows must be at least 1\n"; return 2; }
    try {
        HaplotypeFixture fx(hapFile);
        std::vector<int> indices, lines;
        fx.listWindows(indices, lines);
        for (size_t k = 0; k < indices.size(); k++) {       // every window first: nothing is written for an input that cannot be finished
            const bool noRef = fx.find(indices[k])->refSeq.empty();
            fx.release(indices[k]);
            if (noRef) {
                std::cerr << "dindel_hapalign: window " << indices[k] << " has no R record (W record in line " << lines[k] << " of " << hapFile << ")\n";
                return 1;
            }
        }
        std::ofstream out(outFile.c_str());
        if (!out) throw std::string("Cannot open output file ").append(outFile);
        size_t nHaps = 0, nKept = 0;
        for (size_t w0 = 0; w0 < indices.size(); w0 += size_t(batchWindows)) {
            const size_t w1 = std::min(indices.size(), w0 + size_t(batchWindows));
            std::vector<WindowHaplotypes> wins;
            std::vector<std::string> refs;
            for (size_t k = w0; k < w1; k++) {
                const WindowHaplotypes *w = fx.find(indices[k]);
                WindowHaplotypes in;
                in.index = w->index; in.leftPos = w->leftPos; in.rightPos = w->rightPos;
                for (size_t h = 0; h < w->haps.size(); h++) in.haps.push_back(Haplotype(w->haps[h].seq));   // A / V records of the input are ignored
                nHaps += in.haps.size();
                wins.push_back(in);
                refs.push_back(w->refSeq);
                fx.release(indices[k]);
            }
            alignHaplotypesBatch(wins, refs, device, NULL, hostConvert ? CONVERT_HOST : CONVERT_DEVICE, true);    // (the A records need refHpos)
            for (size_t k = 0; k < wins.size(); k++) { nKept += wins[k].haps.size(); writeWindow(out, wins[k]); }
            if (!quiet) std::cerr << "dindel_hapalign: " << w1 << " of " << indices.size() << " windows\n";
        }
        out.flush();
        if (!out) throw std::string("Cannot write output file ").append(outFile);
        if (!quiet) std::cerr << "dindel_hapalign: " << indices.size() << " windows, " << nHaps << " haplotypes in, " << nKept << " out\n";
    } catch (std::string &e) {
        std::cerr << "dindel_hapalign: " << e << "\n";
        return 1;
    } catch (HaplotypeFixture::Error &e) {
        std::cerr << "dindel_hapalign: " << e.message << "\n";
        return 1;
    }
    return 0;
}
