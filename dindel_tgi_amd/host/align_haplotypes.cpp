// align_haplotypes.cpp — see align_haplotypes.hpp.  The alignment itself (SeqAn globalAlignment in the reference) is the device's; this
// file restates what the reference does with it, quirks included.
#include <algorithm>
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

static void finishWindowTail(WindowHaplotypes &w, const std::vector<bool> &startEnd, std::vector<int> *kept);

void finishWindowHaplotypes(WindowHaplotypes &w, const std::string &refSeq, const std::vector<std::vector<int> > &refPos, std::vector<int> *kept)
{
    if (refPos.size() != w.haps.size()) throw std::string("finishWindowHaplotypes: one alignment per haplotype is required");
    std::vector<bool> startEnd(w.haps.size(), false);
    for (size_t h = 0; h < w.haps.size(); h++) {
        Haplotype &hap = w.haps[h];
        convertHaplotypeAlignment(refSeq, hap, refPos[h]);
        bool hasStartEndIndel = false;
        if (!hap.refHpos.empty() && hap.refHpos[0] == MLAlignment::LO) hasStartEndIndel = true;
        const int hs = int(hap.refHpos.size()) - 1;
        if (hs > 0 && hap.refHpos[hs] == MLAlignment::RO) hasStartEndIndel = true;
        startEnd[h] = hasStartEndIndel;
    }
    finishWindowTail(w, startEnd, kept);
}

// what alignHaplotypes and getHaplotypes do once every haplotype has its variants; startEnd[h]: the overhang test of DInDel.cpp:1488-1491
static void finishWindowTail(WindowHaplotypes &w, const std::vector<bool> &startEnd, std::vector<int> *kept)
{
    // reference DInDel.cpp:1452-1505: variants are collected by position from every haplotype, also from those that are dropped
    std::set<int> positions;
    std::vector<Haplotype> tmp;
    std::vector<int> tmpIdx;
    for (size_t h = 0; h < w.haps.size(); h++) {
        const Haplotype &hap = w.haps[h];
        for (std::map<int, AlignedVariant>::const_iterator it = hap.indels.begin(); it != hap.indels.end(); ++it) positions.insert(it->first);
        for (std::map<int, AlignedVariant>::const_iterator it = hap.snps.begin(); it != hap.snps.end(); ++it) positions.insert(it->first);
        if (!startEnd[h]) { tmp.push_back(hap); tmpIdx.push_back(int(h)); }
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

// ---- the variants kernel's twin (csrc/hap_variants_kernel.hip): the walk of convertHaplotypeAlignment on the slice itself and the flank
//      loops of getFlankingCoordinatesBetter in closed form.  The derivation is in the kernel's header comment. ----
namespace {

struct FlankSeqs { const char *ref; int S; const char *hap; };

// length of the run of positions, counted from `from` in steps of `step` while `inside`, at which the two letters agree
template <class Eq> int equalRun(int from, int step, int lo, int hi, Eq eq)
{
    int n = 0;
    for (int j = from; j >= lo && j <= hi && eq(j); j += step) n++;
    return n;
}

void setFlanks(dd_hap_variant &v, int sh, int rlen, int lfh, int rfh, int rightOfRead)
{
    if (lfh <= 0) lfh = 0;
    int lfr = v.start_read - (sh - lfh) + 1;
    if (lfr < 0) lfr = 0;
    const int rfr = rightOfRead + (rfh - sh);
    if (rfr >= rlen) lfr = rlen - 1;
    v.left_flank_hap = int16_t(lfh); v.right_flank_hap = int16_t(rfh); v.left_flank_read = int16_t(lfr); v.right_flank_read = int16_t(rfr);
}

void deletionFlanks(const FlankSeqs &q, int rlen, dd_hap_variant &v)
{
    const int sh = v.key, l = v.len, S = q.S;
    const int runL = equalRun(sh - 1, -1, 1, S, [&](int j) { return q.ref[j] == q.ref[j + l]; });
    const int runR = equalRun(sh, 1, 0, S - l - 1, [&](int i) { return q.ref[i] == q.ref[i + l]; });
    const int xmax = std::max(sh, std::min(sh + runR, S - l - 1));
    setFlanks(v, sh, rlen, sh - runL - 1, xmax + l, v.start_read + 1 - l);
}

// false: no closed form for this insertion (at least as long as the reference sequence)
bool insertionFlanks(const FlankSeqs &q, int rlen, dd_hap_variant &v)
{
    const int sh = v.key, l = v.len, S = q.S;
    if (l >= S) return false;
    auto O = [&](int k) { return k < sh ? q.ref[k] : k < sh + l ? dnaLetter(q.hap[v.start_read + (k - sh)]) : q.ref[k - l]; };   // the reference with the insertion in place
    const int runL = equalRun(sh - 1, -1, 1, S, [&](int j) { return q.ref[j] == O(j + l); });
    const int runR = equalRun(sh, 1, 0, S - 1, [&](int i) { return q.ref[i] == O(i); });
    const int xmax = std::max(sh, std::min(sh + runR, S - l - 1));
    setFlanks(v, sh, rlen, sh - runL - 1, xmax, v.start_read + l);
    return true;
}

void snpFlanks(int S, int rlen, dd_hap_variant &v)
{
    int lfr = v.start_read - 1; if (lfr < 0) lfr = 0;
    const int rfr = v.start_read + 1; if (rfr >= rlen) lfr = rlen - 1;
    int lfh = v.key - 1; if (lfh < 0) lfh = 0;
    const int rfh = v.key + 1; if (rfh >= S) lfh = S - 1;
    v.left_flank_hap = int16_t(lfh); v.right_flank_hap = int16_t(rfh); v.left_flank_read = int16_t(lfr); v.right_flank_read = int16_t(rfr);
}

} // namespace

void hapVariantsHost(const dd_align_batch &b, const int32_t *status, const int16_t *refPos, dd_hap_variants_summary *summary, dd_hap_variant *variants, int cap)
{
    for (int pair = 0; pair < b.n_pairs; pair++) {
        dd_hap_variants_summary &sum = summary[pair];
        sum.n_variants = sum.first_base = sum.last_base = sum.flags = 0;
        const int r = b.pair_ref[pair];
        if (status[pair] != DD_ALIGN_OK || r < 0 || r >= b.n_refs) continue;
        const int h0 = b.hap_off[pair], rlen = b.hap_off[pair + 1] - h0, S = b.ref_off[r + 1] - b.ref_off[r];
        const FlankSeqs q = { b.ref_seq + b.ref_off[r], S, b.hap_seq + h0 };
        const int16_t *rp = refPos + h0;
        dd_hap_variant *out = variants + size_t(pair) * size_t(cap);
        int n = 0, nxt = 0, fb = -1;
        auto put = [&](const dd_hap_variant &v) { if (n < cap) out[n] = v; n++; };
        for (int x = 0; x < rlen;) {
            const int p = rp[x], upto = p < 0 ? -1 - p : p;
            if (upto > nxt) {                                      // deleted reference bases in front of base x
                dd_hap_variant v = { int16_t(fb >= 0 ? DD_ALIGN_EVENT_DEL : DD_HAP_VARIANT_DEL_UNSEEN), int16_t(nxt), int16_t(upto - nxt), int16_t(x - 1), 0, 0, 0, 0 };
                if (fb >= 0) deletionFlanks(q, rlen, v);
                put(v);
            }
            if (p >= 0) {
                if (fb < 0) fb = p;
                if (dnaLetter(q.hap[x]) != dnaLetter(q.ref[p])) {
                    dd_hap_variant v = { DD_HAP_VARIANT_SNP, int16_t(p), 1, int16_t(x), 0, 0, 0, 0 };
                    snpFlanks(S, rlen, v);
                    put(v);
                }
                nxt = p + 1; x++;
                continue;
            }
            int run = 1;
            while (x + run < rlen && rp[x + run] == p) run++;       // gap-facing bases with one upto: LO, an insertion, or RO
            if (upto > 0 && upto < S) {
                dd_hap_variant v = { DD_ALIGN_EVENT_INS, int16_t(upto), int16_t(run), int16_t(x), 0, 0, 0, 0 };
                if (!insertionFlanks(q, rlen, v)) sum.flags |= DD_HAP_VARIANTS_HOST;
                put(v);
            }
            nxt = upto; x += run;
        }
        sum.n_variants = n; sum.first_base = fb; sum.last_base = nxt;
        if (rp[0] == -1) sum.flags |= DD_HAP_VARIANTS_LO_FIRST;
        if (rlen > 1 && rp[rlen - 1] < 0 && -1 - rp[rlen - 1] == S) sum.flags |= DD_HAP_VARIANTS_RO_LAST;
    }
}

void haplotypeFromVariants(const std::string &refSeq, Haplotype &hap, const dd_hap_variant *v, int n)
{
    hap.indels.clear(); hap.snps.clear();
    hap.align = std::string(refSeq.size(), 'R');
    for (int k = 0; k < n; k++) {
        const dd_hap_variant &x = v[k];
        if (x.kind == DD_ALIGN_EVENT_DEL || x.kind == DD_HAP_VARIANT_DEL_UNSEEN) {
            std::string seq("-");
            for (int i = 0; i < x.len; i++) { seq += dnaLetter(refSeq[size_t(x.key + i)]); hap.align[size_t(x.key + i)] = 'D'; }
            if (x.kind == DD_HAP_VARIANT_DEL_UNSEEN) continue;
            AlignedVariant av(seq, x.key, x.key + x.len - 1, x.start_read, x.start_read + 1);
            av.setFlanking(x.left_flank_hap, x.right_flank_hap, x.left_flank_read, x.right_flank_read);
            hap.indels[x.key] = av;
        } else if (x.kind == DD_ALIGN_EVENT_INS) {
            std::string seq("+");
            for (int i = 0; i < x.len; i++) seq += dnaLetter(hap.seq[size_t(x.start_read + i)]);
            AlignedVariant av(seq, x.key, x.key, x.start_read, x.start_read + x.len - 1);
            av.setFlanking(x.left_flank_hap, x.right_flank_hap, x.left_flank_read, x.right_flank_read);
            hap.indels[x.key] = av;
        } else {
            std::string snp("X=>X");
            snp[0] = dnaLetter(refSeq[size_t(x.key)]); snp[3] = dnaLetter(hap.seq[size_t(x.start_read)]);
            AlignedVariant av(snp, x.key, x.key, x.start_read, x.start_read);
            av.setFlanking(x.left_flank_hap, x.right_flank_hap, x.left_flank_read, x.right_flank_read);
            hap.snps[x.key] = av;
            hap.align[size_t(x.key)] = snp[3];
        }
    }
}

void refHposFromSlice(int hlen, const int16_t *refPos, int rlen, std::vector<int> &refHpos)
{
    refHpos.resize(size_t(rlen));
    for (int b = 0; b < rlen; b++) {
        const int p = refPos[b];
        refHpos[size_t(b)] = p >= 0 ? p : p == -1 ? int(MLAlignment::LO) : -1 - p < hlen ? int(MLAlignment::INS) : int(MLAlignment::RO);
    }
}

void finishWindowHaplotypesFromVariants(WindowHaplotypes &w, const std::string &refSeq, const dd_hap_variants_summary *summary, const dd_hap_variant *variants,
                                        int cap, const std::vector<const int16_t *> &slices, std::vector<int> *kept)
{
    if (slices.size() != w.haps.size()) throw std::string("finishWindowHaplotypesFromVariants: one slice pointer (or NULL) per haplotype is required");
    std::vector<bool> startEnd(w.haps.size(), false);
    for (size_t h = 0; h < w.haps.size(); h++) {
        Haplotype &hap = w.haps[h];
        const dd_hap_variants_summary &sum = summary[h];
        if ((sum.flags & DD_HAP_VARIANTS_HOST) || sum.n_variants > cap) {
            if (!slices[h]) throw std::string("finishWindowHaplotypesFromVariants: a pair that must be converted on the host came without its slice");
            convertHaplotypeAlignment(refSeq, hap, std::vector<int>(slices[h], slices[h] + hap.seq.size()));
        } else {
            haplotypeFromVariants(refSeq, hap, variants + h * size_t(cap), sum.n_variants);
            if (slices[h]) refHposFromSlice(int(refSeq.size()), slices[h], int(hap.seq.size()), hap.refHpos);
            else hap.refHpos.clear();
        }
        startEnd[h] = (sum.flags & (DD_HAP_VARIANTS_LO_FIRST | DD_HAP_VARIANTS_RO_LAST)) != 0;
    }
    finishWindowTail(w, startEnd, kept);
}

void alignHaplotypesBatch(std::vector<WindowHaplotypes> &wins, const std::vector<std::string> &refSeqs, int device, std::vector<std::string> *errors,
                          ConvertMode mode, bool needRefHpos)
{
    if (errors) errors->assign(wins.size(), std::string());
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
    const bool records = mode == CONVERT_DEVICE;
    const int cap = kHapVariantsCap;
    std::vector<int32_t> score(nPairs ? nPairs : 1), status(nPairs ? nPairs : 1);
    std::vector<int16_t> refPos;
    std::vector<dd_hap_variants_summary> summary(records ? nPairs : 0);
    std::vector<dd_hap_variant> variants(records ? nPairs * size_t(cap) : 0);
    bool haveSlice = !records || needRefHpos;
    if (haveSlice) refPos.resize(hapAll.size() ? hapAll.size() : 1);
    if (nPairs) {
        dd_align_batch b;
        b.n_refs = int32_t(wins.size()); b.ref_off = refOff.data(); b.ref_seq = refAll.data();
        b.n_pairs = int32_t(nPairs); b.pair_ref = pairRef.data(); b.hap_off = hapOff.data(); b.hap_seq = hapAll.data();
        dd_align_result r = { score.data(), status.data(), haveSlice ? refPos.data() : NULL };
        if (!records) { if (dd_align_haplotypes(&b, &r, device) != DD_SUCCESS) throw std::string("dd_align_haplotypes: ") + dd_last_error(); }
        else {
            if (dd_align_haplotypes_variants(&b, &r, summary.data(), variants.data(), cap, device) != DD_SUCCESS)
                throw std::string("dd_align_haplotypes_variants: ") + dd_last_error();
            bool hostPair = false;
            for (size_t k = 0; k < nPairs && !hostPair; k++) hostPair = (summary[k].flags & DD_HAP_VARIANTS_HOST) || summary[k].n_variants > cap;
            if (hostPair && !haveSlice) {                  // rare: the slices after all, by the plain entry
                refPos.resize(hapAll.size() ? hapAll.size() : 1);
                r.ref_pos = refPos.data();
                if (dd_align_haplotypes(&b, &r, device) != DD_SUCCESS) throw std::string("dd_align_haplotypes: ") + dd_last_error();
                haveSlice = true;
            }
        }
    }
    size_t pair = 0;
    for (size_t w = 0; w < wins.size(); w++) {
        const size_t pair0 = pair;
        std::vector<std::vector<int> > pos(records ? 0 : wins[w].haps.size());
        std::vector<const int16_t *> slices(records ? wins[w].haps.size() : 0, (const int16_t *)NULL);
        std::string error;
        for (size_t h = 0; h < wins[w].haps.size(); h++, pair++) {
            if (status[pair] != DD_ALIGN_OK && error.empty()) {
                std::ostringstream os;
                os << "haplotype " << h << " of window " << wins[w].index << " cannot be aligned: "
                   << (status[pair] == DD_ALIGN_EMPTY ? "empty haplotype or reference sequence" : "sequence longer than 4094 bases");
                if (!errors) throw os.str();
                error = os.str();
            }
            if (!records) pos[h].assign(refPos.begin() + hapOff[pair], refPos.begin() + hapOff[pair + 1]);
            else if (haveSlice) slices[h] = refPos.data() + hapOff[pair];
        }
        if (!error.empty()) { (*errors)[w] = error; wins[w].haps.clear(); continue; }
        try {
            if (!records) finishWindowHaplotypes(wins[w], refSeqs[w], pos);
            else finishWindowHaplotypesFromVariants(wins[w], refSeqs[w], summary.data() + pair0, variants.data() + pair0 * size_t(cap), cap, slices);
        } catch (std::string &e) { if (!errors) throw; (*errors)[w] = e; wins[w].haps.clear(); }
    }
}

} // namespace dindel
