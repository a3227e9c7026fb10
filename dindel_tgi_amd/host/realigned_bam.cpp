// realigned_bam.cpp — see realigned_bam.hpp.  Line references are to the reference's DInDel.cpp.
#include "realigned_bam.hpp"
#include "../../include/dindel_hmm.h"
#include <algorithm>
#include <cmath>
#include <sstream>

namespace dindel {

namespace {
struct PairLik { double ll; int h1, h2; };
bool byLikDescending(const PairLik &a, const PairLik &b) { return a.ll > b.ll; }             // :3826-3831
}

std::pair<int, int> maxLikelihoodPairOf(size_t lh, size_t numReads, const std::function<double(size_t, size_t)> &ll,
                                        const std::function<double(size_t, size_t)> &prior, std::vector<double> *values)
{
    std::vector<PairLik> likPairs;                                                           // :3767-3824 (the counters of HapPairLik are not read here)
    if (values) values->assign(lh * lh, 0.0);
    for (size_t hp = 0; hp < lh; hp++) for (size_t hm = hp; hm < lh; hm++) {
        double l = 0.0;
        for (size_t r = 0; r < numReads; r++) l += (addLogs(ll(hp, r), ll(hm, r)) + log(.5));
        l += prior(hp, hm);                                                                  // usePrior = true at :591
        PairLik p = { l, int(hp), int(hm) };
        likPairs.push_back(p);
        if (values) (*values)[hp * lh + hm] = l;
    }
    // the reference sorts its HapPairLik records with std::sort and this comparator; the order of equal likelihoods is the
    // algorithm's, which depends on the comparisons alone — the same here
    std::sort(likPairs.begin(), likPairs.end(), byLikDescending);
    size_t midx = likPairs.size();                                                           // getMaxHap, :292-300
    double maxll = -HUGE_VAL;
    for (size_t idx = 0; idx < likPairs.size(); idx++) if (likPairs[idx].ll > maxll) { maxll = likPairs[idx].ll; midx = idx; }
    if (midx == likPairs.size()) throw std::string("no haplotype pair with a finite likelihood");   // the reference reads an uninitialised index
    return std::pair<int, int>(likPairs[midx].h1, likPairs[midx].h2);
}

std::pair<int, int> maxLikelihoodPair(const std::vector<Haplotype> &haps, const std::vector<Read> &reads, const WindowLikelihoods &liks,
                                      int leftPos, const AlignedCandidates &candidateVariants, const DiploidParameters &params)
{
    return maxLikelihoodPairOf(haps.size(), reads.size(), [&](size_t h, size_t r) { return liks.ll(h, r); },
                               [&](size_t hp, size_t hm) { return getHaplotypePrior(haps[hp], haps[hm], leftPos, candidateVariants, params); }, NULL);
}

void realignedCigars(const std::vector<Haplotype> &haps, const std::vector<Read> &reads, const WindowLikelihoods &liks, std::pair<int, int> pair,
                     int refSeqPos, std::vector<CIGAR> &cigars)
{
    cigars.assign(reads.size(), CIGAR());
    const size_t h1 = size_t(pair.first), h2 = size_t(pair.second);
    for (size_t r = 0; r < reads.size(); r++) {                                              // :596-611
        size_t hmax = h1;
        if (fabs(liks.ll(h1, r) - liks.ll(h2, r)) < 1e-8) {
            if (haps[h1].countIndels() < haps[h2].countIndels()) hmax = h1; else hmax = h2;
        } else {
            if (liks.ll(h1, r) > liks.ll(h2, r)) hmax = h1; else hmax = h2;
        }
        const MLAlignment ml = liks.get(hmax, r);
        cigars[r] = getCIGAR(haps[hmax].refHpos, haps[hmax].size(), ml, reads[r].size(), refSeqPos);
    }
}

namespace {
// One row of a device result block — the per-pair CIGARs' (setDeviceCigars) or the realigned reads' (setDeviceRealign) — as the CIGAR of
// pair (h, r); a read over the batch's cap (DD_CIGAR_OVERFLOW, or a pair the device did not compute) on the host, from the window's
// alignments, which `full` keeps once they were asked for.
struct DeviceCigarRow { int status, n; const uint32_t *ops; int refOff; };
CIGAR cigarOfRow(const DeviceCigarRow &row, const std::vector<Haplotype> &haps, const std::vector<Read> &reads, size_t h, size_t r, int refSeqPos,
                 WindowLikelihoods &full, const std::function<WindowLikelihoods()> &withAlignments, long *hostFallbacks)
{
    static const char *const thrown[] = {"", "Haplotype has not been aligned!", "Error(1)!", "Error(2)!", "Error(3)!", "Error(4)!", "How is this possible? (1)"};
    const int st = row.status;
    if (st >= DD_CIGAR_HAP_NOT_ALIGNED && st <= DD_CIGAR_IMPOSSIBLE) throw std::string(thrown[st]);
    if (st == DD_CIGAR_OK) {
        const uint32_t *ops = row.ops;
        const int n = row.n, off = row.refOff;
        CIGAR c;
        for (int i = 0; i < n; i++) c.push_back(CIGAR::CIGOp(int(ops[i] & 15u), int(ops[i] >> 4)));
        c.refPos = off < 0 ? -1 : refSeqPos + off;                                           // no aligned base: refPos stays -1
        return c;
    }
    if (!full.valid()) {
        if (!withAlignments) throw std::string("realignedCigars: a read needs the host getCIGAR and no alignments are at hand");
        full = withAlignments();
    }
    const CIGAR c = getCIGAR(haps[h].refHpos, haps[h].size(), full.get(h, r), reads[r].size(), refSeqPos);
    if (hostFallbacks) ++*hostFallbacks;
    return c;
}
CIGAR deviceCigarOf(const std::vector<Haplotype> &haps, const std::vector<Read> &reads, const WindowLikelihoods &liks, size_t h, size_t r, int refSeqPos,
                    WindowLikelihoods &full, const std::function<WindowLikelihoods()> &withAlignments, long *hostFallbacks)
{
    const DeviceCigarRow row = {liks.cigarStatus(h, r), liks.cigarNumOps(h, r), liks.cigarOps(h, r), liks.cigarRefOff(h, r)};
    return cigarOfRow(row, haps, reads, h, r, refSeqPos, full, withAlignments, hostFallbacks);
}
}

void realignedCigars(const std::vector<Haplotype> &haps, const std::vector<Read> &reads, const WindowLikelihoods &liks, std::pair<int, int> pair,
                     int refSeqPos, std::vector<CIGAR> &cigars, const std::function<WindowLikelihoods()> &withAlignments, long *hostFallbacks)
{
    if (!liks.hasDeviceCigars()) { realignedCigars(haps, reads, liks, pair, refSeqPos, cigars); return; }
    cigars.assign(reads.size(), CIGAR());
    const size_t h1 = size_t(pair.first), h2 = size_t(pair.second);
    WindowLikelihoods full;
    for (size_t r = 0; r < reads.size(); r++) {                                              // :596-611
        size_t hmax = h1;
        if (fabs(liks.ll(h1, r) - liks.ll(h2, r)) < 1e-8) {
            if (haps[h1].countIndels() < haps[h2].countIndels()) hmax = h1; else hmax = h2;
        } else {
            if (liks.ll(h1, r) > liks.ll(h2, r)) hmax = h1; else hmax = h2;
        }
        cigars[r] = deviceCigarOf(haps, reads, liks, hmax, r, refSeqPos, full, withAlignments, hostFallbacks);
    }
}

void pooledRealignedCigars(size_t numHaps, size_t numReads, const std::function<double(size_t, size_t)> &ll, const std::function<bool(size_t)> &onHap,
                           const std::function<CIGAR(size_t, size_t)> &cigarOf, std::vector<CIGAR> &cigars)
{
    cigars.assign(numReads, CIGAR());                                                        // :502
    for (size_t r = 0; r < numReads; r++) {
        if (!onHap(r)) continue;                                                             // :504
        double llmax = -HUGE_VAL;                                                            // :505-510
        size_t hidx = 0;
        for (size_t h = 0; h < numHaps; h++) {
            const double l = ll(h, r);
            if (l > llmax) { llmax = l; hidx = h; }
        }
        cigars[r] = cigarOf(hidx, r);                                                        // :511
    }
}

void pooledRealignedCigars(const std::vector<Haplotype> &haps, const std::vector<Read> &reads, const WindowLikelihoods &liks, int refSeqPos,
                           std::vector<CIGAR> &cigars)
{
    pooledRealignedCigars(haps.size(), reads.size(), [&](size_t h, size_t r) { return liks.ll(h, r); }, [&](size_t r) { return liks.onHap(r) != 0; },
                          [&](size_t h, size_t r) { return getCIGAR(haps[h].refHpos, haps[h].size(), liks.get(h, r), reads[r].size(), refSeqPos); }, cigars);
}

void pooledRealignedCigars(const std::vector<Haplotype> &haps, const std::vector<Read> &reads, const WindowLikelihoods &liks, int refSeqPos,
                           std::vector<CIGAR> &cigars, const std::function<WindowLikelihoods()> &withAlignments, long *hostFallbacks)
{
    if (liks.hasDeviceRealign()) { pooledDeviceRealignedCigars(haps, reads, liks, refSeqPos, cigars, withAlignments, hostFallbacks); return; }
    if (!liks.hasDeviceCigars()) { pooledRealignedCigars(haps, reads, liks, refSeqPos, cigars); return; }
    WindowLikelihoods full;
    pooledRealignedCigars(haps.size(), reads.size(), [&](size_t h, size_t r) { return liks.ll(h, r); }, [&](size_t r) { return liks.onHap(r) != 0; },
                          [&](size_t h, size_t r) { return deviceCigarOf(haps, reads, liks, h, r, refSeqPos, full, withAlignments, hostFallbacks); }, cigars);
}

void pooledDeviceRealignedCigars(const std::vector<Haplotype> &haps, const std::vector<Read> &reads, const WindowLikelihoods &liks, int refSeqPos,
                                 std::vector<CIGAR> &cigars, const std::function<WindowLikelihoods()> &withAlignments, long *hostFallbacks)
{
    if (!liks.hasDeviceRealign()) throw std::string("pooledDeviceRealignedCigars: the batch was run without device realign");
    cigars.assign(reads.size(), CIGAR());                                                    // :502
    WindowLikelihoods full;
    for (size_t r = 0; r < reads.size(); r++) {                                              // reads in order: a throw is the first read's that throws
        const int st = liks.realignStatus(r);
        if (st == DD_REALIGN_OFF_HAP || st == DD_REALIGN_NO_HAPS) continue;                  // :504 (without haplotypes no read is on one)
        const int h = liks.realignHap(r);
        if (st == DD_REALIGN_BAD_PAIR || h < 0 || size_t(h) >= haps.size()) throw std::string("pooledDeviceRealignedCigars: no haplotype was chosen for a read");
        const DeviceCigarRow row = {st, liks.realignNumOps(r), liks.realignOps(r), liks.realignRefOff(r)};
        cigars[r] = cigarOfRow(row, haps, reads, size_t(h), r, refSeqPos, full, withAlignments, hostFallbacks);   // :511
    }
}

std::pair<int, int> diploidDeviceRealignedCigars(const std::vector<Haplotype> &haps, const std::vector<Read> &reads, const WindowLikelihoods &liks, int leftPos,
                                                 const AlignedCandidates &candidateVariants, const DiploidParameters &params, int refSeqPos,
                                                 std::vector<CIGAR> &cigars, const std::function<WindowLikelihoods()> &withAlignments, long *hostFallbacks,
                                                 long *uncertifiedWindows)
{
    if (!liks.hasDevicePair() || !liks.hasDeviceRealign()) throw std::string("diploidDeviceRealignedCigars: the batch was run without the device pair");
    if (liks.pairState() != DD_DIPPAIR_CERTIFIED) {                                          // the host's window, as without the switch (:589-611)
        if (uncertifiedWindows) ++*uncertifiedWindows;
        const std::pair<int, int> best = maxLikelihoodPair(haps, reads, liks, leftPos, candidateVariants, params);
        if (!withAlignments) throw std::string("diploidDeviceRealignedCigars: a window needs the host's CIGARs and no alignments are at hand");
        const WindowLikelihoods full = withAlignments();
        realignedCigars(haps, reads, full, best, refSeqPos, cigars);
        return best;
    }
    const std::pair<int, int> pair = liks.devicePair();
    cigars.assign(reads.size(), CIGAR());
    WindowLikelihoods full;
    for (size_t r = 0; r < reads.size(); r++) {                                              // reads in order: a throw is the first read's that throws
        const int st = liks.realignStatus(r), h = liks.realignHap(r);
        if (h < 0 || (h != pair.first && h != pair.second) || size_t(h) >= haps.size())
            throw std::string("diploidDeviceRealignedCigars: a read of a certified window has no haplotype of its pair");
        const DeviceCigarRow row = {st, liks.realignNumOps(r), liks.realignOps(r), liks.realignRefOff(r)};
        cigars[r] = cigarOfRow(row, haps, reads, size_t(h), r, refSeqPos, full, withAlignments, hostFallbacks);
    }
    return pair;
}

std::string realignedBAMFileName(const std::string &prefix, int index, const std::string &tid, uint32_t leftPos, uint32_t rightPos, int minReadOverlap)
{
    std::stringstream os;                                                                    // :614-618
    os << index << "_" << tid << "_" << leftPos + uint32_t(minReadOverlap) << "_" << rightPos - uint32_t(minReadOverlap) << ".bam";
    return std::string(prefix).append(".ra.").append(os.str());
}

void writeRealignedBAMFile(const std::string &fileName, const std::vector<CIGAR> &cigars, const std::vector<Read> &reads, const std::vector<int> &onHap,
                           const BamFile &header)
{
    if (cigars.size() != reads.size()) throw std::string("Problem with the cigars.");        // :672
    BamWriter out(fileName, header);                                                         // bam_open + bam_header_write, :674-680
    std::vector<uint8_t> nb;
    for (size_t r = 0; r < reads.size(); r++) {
        if (!reads[r].record) throw std::string("Read has no BAM record.");
        const std::vector<uint8_t> &b = *reads[r].record;
        if (onHap[r]) {                                                                      // :686-718
            const uint32_t l_qname = b[8];
            const uint32_t old_ncig = uint32_t(b[12]) | (uint32_t(b[13]) << 8);
            const uint32_t new_ncig = uint32_t(cigars[r].size());
            nb.assign(b.begin(), b.begin() + 32 + long(l_qname));                            // the fixed fields and the name
            for (uint32_t n = 0; n < new_ncig; n++) {
                const uint32_t v = (uint32_t(cigars[r][n].second) << 4) | uint32_t(cigars[r][n].first);     // length << BAM_CIGAR_SHIFT | operation
                nb.push_back(uint8_t(v)); nb.push_back(uint8_t(v >> 8)); nb.push_back(uint8_t(v >> 16)); nb.push_back(uint8_t(v >> 24));
            }
            nb.insert(nb.end(), b.begin() + 32 + long(l_qname) + 4 * long(old_ncig), b.end());   // bases, qualities, tags
            nb[12] = uint8_t(new_ncig); nb[13] = uint8_t(new_ncig >> 8);                       // core.n_cigar (16 bits)
            const int32_t pos = int32_t(cigars[r].refPos);                                   // core.pos, :712
            const int32_t mpos = int32_t(uint32_t(b[24]) | (uint32_t(b[25]) << 8) | (uint32_t(b[26]) << 16) | (uint32_t(b[27]) << 24));
            const int32_t isize = pos - mpos;                                                // :714
            for (int k = 0; k < 4; k++) { nb[4 + size_t(k)] = uint8_t(uint32_t(pos) >> (8 * k)); nb[28 + size_t(k)] = uint8_t(uint32_t(isize) >> (8 * k)); }
            out.write(nb);
        } else out.write(b);                                                                 // :720
    }
    out.close();
}

} // namespace dindel
