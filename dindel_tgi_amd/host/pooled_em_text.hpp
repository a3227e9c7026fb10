// pooled_em_text.hpp — one window of the pooled analysis written as text, for the checks that run host/pooled_em.cpp without a device
// (pooled_capi.cpp for the pytest suite, tests/pooled_em_check.cpp under the sanitizers).  Records, one per line:
//   W index tid leftPos rightPos candPos numPools
//   C pos str freq              a candidate of the window file (absolute position; freq < 0: none given)
//   H filtered                  the next haplotype;   V key str   an entry of its variant map (position in the window, string)
//   R pool reverse mapQual unmapped                    the next read
//   L h r ll offHap             one record;   K h r pos snp   its covered flag at `pos` is set (snp 1: hapSNPCovered)
//   X pos str nf nr             filterHaplotypes' coverage of a variant
// pooledLinesOfText runs plan, EM (dd_pooled_em_host) and lines, and returns the lines.
#ifndef DINDEL_POOLED_EM_TEXT_HPP
#define DINDEL_POOLED_EM_TEXT_HPP
#include <set>
#include <sstream>
#include "pooled_em.hpp"

namespace dindel {

inline std::string pooledLinesOfText(const std::string &text, const std::string &program, double a0, double priorSNP, double priorIndel)
{
    std::istringstream is(text);
    std::string line, tid = "NA";
    int index = 0;
    uint32_t leftPos = 0, rightPos = 0, candPos = 0;
    size_t numPools = 1;
    std::vector<AlignedVariant> cands;
    std::vector<Haplotype> haps;
    std::vector<Read> reads;
    PooledWindow win;
    struct Rec { size_t h, r; double ll; int off; };
    std::vector<Rec> recs;
    std::shared_ptr<std::set<std::vector<long> > > covered(new std::set<std::vector<long> >());
    while (std::getline(is, line)) {
        std::istringstream ls(line);
        std::string kind, str;
        if (!(ls >> kind)) continue;
        if (kind == "W") ls >> index >> tid >> leftPos >> rightPos >> candPos >> numPools;
        else if (kind == "C") { int pos; double freq; ls >> pos >> str >> freq; cands.push_back(AlignedVariant(str, pos, freq)); }
        else if (kind == "H") { int f; ls >> f; haps.push_back(Haplotype()); win.filtered.push_back(f); }
        else if (kind == "V") { int key; ls >> key >> str; if (haps.empty()) throw std::string("V before H"); haps.back().indels[key] = AlignedVariant(str, key, key, -1, -1); }
        else if (kind == "R") { Read rd; int rev, unm; ls >> rd.poolID >> rev >> rd.mapQual >> unm; rd.onReverseStrand = rev != 0; rd.unmapped = unm != 0; reads.push_back(rd); }
        else if (kind == "L") { Rec x; ls >> x.h >> x.r >> x.ll >> x.off; recs.push_back(x); }
        else if (kind == "K") { std::vector<long> k(4); ls >> k[0] >> k[1] >> k[2] >> k[3]; covered->insert(k); }
        else if (kind == "X") { int pos, nf, nr; ls >> pos >> str >> nf >> nr; win.varCoverage[PAV(pos, AlignedVariant(str, pos, pos, -1, -1))] = VariantCoverage(nf, nr); }
        else throw std::string("unknown record ").append(kind);
        if (ls.fail()) throw std::string("malformed record: ").append(line);
    }
    win.nh = haps.size(); win.nr = reads.size();
    win.ll.assign(win.nh * win.nr, 0.0); win.offHap.assign(win.nh * win.nr, 0);
    for (size_t i = 0; i < recs.size(); i++) {
        if (recs[i].h >= win.nh || recs[i].r >= win.nr) throw std::string("record outside the window");
        win.ll[recs[i].h * win.nr + recs[i].r] = recs[i].ll; win.offHap[recs[i].h * win.nr + recs[i].r] = uint8_t(recs[i].off != 0);
    }
    for (size_t r = 0; r < reads.size(); r++) if (reads[r].poolID < 0 || size_t(reads[r].poolID) >= numPools) throw std::string("read outside the pools");
    win.covered = [covered](size_t h, size_t r, int pos, bool snp) {
        std::vector<long> k(4); k[0] = long(h); k[1] = long(r); k[2] = pos; k[3] = snp ? 1 : 0;
        return covered->count(k) != 0;
    };
    const AlignedCandidates candidates(tid, cands, int(leftPos), int(rightPos));
    DiploidParameters dip;
    dip.priorSNP = priorSNP; dip.priorIndel = priorIndel;
    PooledParameters pp;
    pp.a0 = a0; pp.bayesType = program;
    PooledPlan plan;
    pooledPlan(haps, win, leftPos, candidates, dip, program, plan);
    pooledRunEM(std::vector<PooledPlan *>(1, &plan), std::vector<const PooledWindow *>(1, &win), pp, true, 0, 1);
    std::ostringstream os;
    OutputData glf = makeGLFOutputData(os);
    pooledLines(haps, reads, win, plan, candPos, leftPos, rightPos, glf, index, tid, candidates, dip, program, numPools);
    return os.str();
}

} // namespace dindel
#endif
