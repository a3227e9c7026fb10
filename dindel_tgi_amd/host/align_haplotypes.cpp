// align_haplotypes.cpp — see align_haplotypes.hpp.  The alignment itself (SeqAn globalAlignment in the reference) is the device's; this
// file restates what the reference does with it, quirks included.
#include <set>
#include <sstream>
#include "align_haplotypes.hpp"
#include "../../include/dindel_hmm.h"

namespace dindel {

char dnaLetter(char c)
{
    switch (c) {
        case 'C': case 'c': return 'C';
        case 'G': case 'g': return 'G';
        case 'T': case 't': case 'U': case 'u': return 'T';
        default: return 'A';
    }
}

// reference ObservationModelSeqAn.hpp:39-138.  Kept as they are: the leftward loops start at sh - 1 and stop at x > 0, and the
// `rightFlankRead >= size` branches assign leftFlankRead (leftFlankHap in the SNP branch).
void getFlankingCoordinatesBetter(const std::string &hapSeq, size_t readSize, AlignedVariant &av)
{
    int rightFlankHap, leftFlankHap, rightFlankRead, leftFlankRead;
    if (av.getType() == AlignedVariant::DEL) {
        const int l = int(av.getSeq().size());
        std::string origSeq = hapSeq;
        const int sh = av.getStartHap();
        origSeq.erase(sh, l);
        leftFlankHap = sh - 1;
        rightFlankHap = sh + l;
        for (int x = sh - 1; x > 0; x--) {
            std::string newseq = hapSeq;
            newseq.erase(x, l);
            if (newseq == origSeq) leftFlankHap = x - 1;
        }
        if (leftFlankHap <= 0) leftFlankHap = 0;
        for (int x = sh + 1; x < int(hapSeq.size() - l); x++) {
            std::string newseq = hapSeq;
            newseq.erase(x, l);
            if (newseq == origSeq) rightFlankHap = x + l;
        }
        leftFlankRead = av.getStartRead() - (sh - leftFlankHap) + 1; if (leftFlankRead < 0) leftFlankRead = 0;
        rightFlankRead = av.getStartRead() + 1 + (rightFlankHap - sh - l); if (rightFlankRead >= int(readSize)) leftFlankRead = int(readSize) - 1;
    } else if (av.getType() == AlignedVariant::INS) {
        const std::string &seq = av.getSeq();
        const int l = int(seq.size());
        std::string origSeq = hapSeq;
        const int sh = av.getStartHap();
        origSeq.insert(sh, seq);
        leftFlankHap = sh - 1;
        rightFlankHap = sh;
        for (int x = sh - 1; x > 0; x--) {
            std::string newseq = hapSeq;
            newseq.insert(x, origSeq.substr(x, l));
            if (newseq == origSeq) leftFlankHap = x - 1;
        }
        if (leftFlankHap <= 0) leftFlankHap = 0;
        for (int x = sh + 1; x < int(hapSeq.size() - l); x++) {
            std::string newseq = hapSeq;
            newseq.insert(x, origSeq.substr(x, l));
            if (newseq == origSeq) rightFlankHap = x;
        }
        leftFlankRead = av.getStartRead() - (sh - leftFlankHap) + 1; if (leftFlankRead < 0) leftFlankRead = 0;
        rightFlankRead = av.getStartRead() + l + (rightFlankHap - sh); if (rightFlankRead >= int(readSize)) leftFlankRead = int(readSize) - 1;
    } else {
        leftFlankRead = av.getStartRead() - 1; if (leftFlankRead < 0) leftFlankRead = 0;
        rightFlankRead = av.getStartRead() + 1; if (rightFlankRead >= int(readSize)) leftFlankRead = int(readSize) - 1;
        leftFlankHap = av.getStartHap() - 1; if (leftFlankHap < 0) leftFlankHap = 0;
        rightFlankHap = av.getStartHap() + 1; if (rightFlankHap >= int(hapSeq.size())) leftFlankHap = int(hapSeq.size()) - 1;
    }
    av.setFlanking(leftFlankHap, rightFlankHap, leftFlankRead, rightFlankRead);
}

// reference ObservationModelSeqAn.hpp:142-269.  There `hap` is the reference sequence (hlen bases, row 0) and `read` the candidate
// haplotype (rlen bases, row 1); the two gapped rows are rebuilt from refPos first, with the letters of the converted bases.  SeqAn writes a
// block substitution as deletion then insertion (the insertion is keyed behind the deleted bases) and an overhang at the matrix edge the
// other way round; refPos carries which.
void convertHaplotypeAlignment(const std::string &refSeq, Haplotype &hap, const std::vector<int> &refPos, int *firstBase, int *lastBase)
{
    const int hlen = int(refSeq.size()), rlen = int(hap.seq.size());
    if (int(refPos.size()) != rlen) throw std::string("convertHaplotypeAlignment: one reference offset per haplotype base is required");
    std::string row0, row1;                       // '-' = gap
    int nxt = 0;                                  // reference bases written so far
    for (int b = 0; b < rlen; b++) {
        const int p = refPos[b];
        const int upto = p >= 0 ? p : -1 - p;     // reference bases in front of this column (DD_ALIGN_GAP_REFS): the deleted ones come first
        if (upto < nxt || upto > hlen - (p >= 0 ? 1 : 0)) throw std::string("convertHaplotypeAlignment: reference offsets must increase within the reference");
        for (; nxt < upto; nxt++) { row0 += dnaLetter(refSeq[nxt]); row1 += '-'; }
        if (p < 0) { row0 += '-'; row1 += dnaLetter(hap.seq[b]); }
        else { row0 += dnaLetter(refSeq[nxt++]); row1 += dnaLetter(hap.seq[b]); }
    }
    for (; nxt < hlen; nxt++) { row0 += dnaLetter(refSeq[nxt]); row1 += '-'; }
    const int end_ = int(row0.size());

    hap.indels.clear(); hap.snps.clear();
    hap.align = std::string(hlen, 'R');
    hap.refHpos.assign(rlen, int(MLAlignment::LO));
    bool fbfound = false;
    int fb = -1;
    int b = 0, rb = 0;
    while (b < end_ && row0[b] == '-') {
        if (row1[b] != '-') { hap.refHpos[rb] = MLAlignment::LO; rb++; }
        ++b;
    }
    int hb = 0;                                   // number of reference bases
    while (b < end_ && rb < rlen) {
        if (row0[b] == '-') {
            if (hb < hlen) {                      // insertion
                std::string seq("+");
                while (b < end_ && row0[b] == '-') { seq += row1[b]; hap.refHpos[rb] = MLAlignment::INS; ++b; ++rb; }
                AlignedVariant av(seq, hb, hb, rb - int(seq.size()) + 1, rb - 1);
                getFlankingCoordinatesBetter(refSeq, hap.seq.size(), av);
                hap.indels[hb] = av;
            } else { hap.refHpos[rb] = MLAlignment::RO; ++rb; ++b; }
        } else if (row1[b] != '-') {
            if (!fbfound) { fbfound = true; fb = hb; }
            if (row1[b] != row0[b]) {             // SNP
                std::string snp("X=>X");
                snp[0] = row0[b]; snp[3] = row1[b];
                AlignedVariant av(snp, hb, hb, rb, rb);
                getFlankingCoordinatesBetter(refSeq, hap.seq.size(), av);
                hap.snps[hb] = av;
                hap.align[hb] = snp[3];
            }
            hap.refHpos[rb] = hb;
            ++rb; ++b; ++hb;
        } else {                                  // deletion: recorded only once the first paired base was seen
            std::string seq("-");
            int len = 0;
            while (b < end_ && row1[b] == '-') { seq += row0[b]; hap.align[hb] = 'D'; ++b; ++hb; ++len; }
            if (fbfound) {
                AlignedVariant av(seq, hb - len, hb - 1, rb - 1, rb);
                getFlankingCoordinatesBetter(refSeq, hap.seq.size(), av);
                hap.indels[hb - len] = av;
            }
        }
    }
    if (firstBase) *firstBase = fb;
    if (lastBase) *lastBase = hb;
}

// reference Haplotype.hpp:201-251
void addRefVariant(Haplotype &hap, int rp)
{
    int offset = 0;
    std::map<int, AlignedVariant>::const_iterator it = hap.indels.begin();
    while (it != hap.indels.end() && it->first <= rp) {
        if (it->second.getType() == AlignedVariant::DEL) {
            if (it->first + it->second.size() <= rp) offset -= it->second.size();
            else break;                           // the deletion deleted rp from the reference
        }
        if (it->second.getType() == AlignedVariant::INS) offset += it->second.size();
        ++it;
    }
    const int readStart = rp + offset, readEnd = rp + offset;
    const char a = hap.align[rp];
    std::string gt = a != 'R' ? std::string("R=>") + a : std::string("*REF");
    if (hap.indels.find(rp) == hap.indels.end()) hap.indels[rp] = AlignedVariant(gt, rp, rp, readStart, readEnd);
    if (hap.snps.find(rp) == hap.snps.end()) hap.snps[rp] = AlignedVariant(gt, rp, rp, readStart, readEnd);
}

void finishWindowHaplotypes(WindowHaplotypes &w, const std::string &refSeq, const std::vector<std::vector<int> > &refPos, std::vector<int> *kept)
{
    if (refPos.size() != w.haps.size()) throw std::string("finishWindowHaplotypes: one alignment per haplotype is required");
    // reference DInDel.cpp:1452-1505: variants are collected by position from every haplotype, also from those that are dropped
    std::set<int> positions;
    std::vector<Haplotype> tmp;
    std::vector<int> tmpIdx;
    for (size_t h = 0; h < w.haps.size(); h++) {
        Haplotype &hap = w.haps[h];
        convertHaplotypeAlignment(refSeq, hap, refPos[h]);
        bool hasStartEndIndel = false;
        if (!hap.refHpos.empty() && hap.refHpos[0] == MLAlignment::LO) hasStartEndIndel = true;
        const int hs = int(hap.refHpos.size()) - 1;
        if (hs > 0 && hap.refHpos[hs] == MLAlignment::RO) hasStartEndIndel = true;
        for (std::map<int, AlignedVariant>::const_iterator it = hap.indels.begin(); it != hap.indels.end(); ++it) positions.insert(it->first);
        for (std::map<int, AlignedVariant>::const_iterator it = hap.snps.begin(); it != hap.snps.end(); ++it) positions.insert(it->first);
        if (!hasStartEndIndel) { tmp.push_back(hap); tmpIdx.push_back(int(h)); }
    }
    // reference DInDel.cpp:1507-1510: the REF allele as a variant of each haplotype, for the coverage statistics
    for (std::set<int>::const_iterator it = positions.begin(); it != positions.end(); ++it)
        for (size_t h = 0; h < tmp.size(); h++) addRefVariant(tmp[h], *it);
    // reference DInDel.cpp:1600-1626: remove duplicate reference haplotypes of different length
    w.haps.clear();
    if (kept) kept->clear();
    bool foundRef = false;
    for (size_t th = 0; th < tmp.size(); th++) {
        if (tmp[th].countIndels() == 0 && tmp[th].countSNPs() == 0) {
            if (foundRef) continue;
            foundRef = true;
        }
        w.haps.push_back(tmp[th]);
        if (kept) kept->push_back(tmpIdx[th]);
    }
}

void alignHaplotypesBatch(std::vector<WindowHaplotypes> &wins, const std::vector<std::string> &refSeqs, int device)
{
    if (wins.size() != refSeqs.size()) throw std::string("alignHaplotypesBatch: one reference sequence per window is required");
    std::vector<int32_t> refOff(1, 0), hapOff(1, 0), pairRef;
    std::string refAll, hapAll;
    for (size_t w = 0; w < wins.size(); w++) {
        refAll += refSeqs[w];
        refOff.push_back(int32_t(refAll.size()));
        for (size_t h = 0; h < wins[w].haps.size(); h++) {
            hapAll += wins[w].haps[h].seq;
            hapOff.push_back(int32_t(hapAll.size()));
            pairRef.push_back(int32_t(w));
        }
    }
    const size_t nPairs = pairRef.size();
    std::vector<int32_t> score(nPairs ? nPairs : 1), status(nPairs ? nPairs : 1);
    std::vector<int16_t> refPos(hapAll.size() ? hapAll.size() : 1);
    if (nPairs) {
        dd_align_batch b;
        b.n_refs = int32_t(wins.size()); b.ref_off = refOff.data(); b.ref_seq = refAll.data();
        b.n_pairs = int32_t(nPairs); b.pair_ref = pairRef.data(); b.hap_off = hapOff.data(); b.hap_seq = hapAll.data();
        dd_align_result r = { score.data(), status.data(), refPos.data() };
        if (dd_align_haplotypes(&b, &r, device) != DD_SUCCESS) throw std::string("dd_align_haplotypes: ") + dd_last_error();
    }
    size_t pair = 0;
    for (size_t w = 0; w < wins.size(); w++) {
        std::vector<std::vector<int> > pos(wins[w].haps.size());
        for (size_t h = 0; h < wins[w].haps.size(); h++, pair++) {
            if (status[pair] != DD_ALIGN_OK) {
                std::ostringstream os;
                os << "haplotype " << h << " of window " << wins[w].index << " cannot be aligned: "
                   << (status[pair] == DD_ALIGN_EMPTY ? "empty haplotype or reference sequence" : "sequence longer than 4094 bases");
                throw os.str();
            }
            pos[h].assign(refPos.begin() + hapOff[pair], refPos.begin() + hapOff[pair + 1]);
        }
        finishWindowHaplotypes(wins[w], refSeqs[w], pos);
    }
}

} // namespace dindel
