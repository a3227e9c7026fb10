// compute_likelihoods.cpp — see compute_likelihoods.hpp.
#include "compute_likelihoods.hpp"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <memory>
#include <mutex>
#include "../../include/dindel_hmm.h"

namespace dindel {

double Read::phredToProb(double phred)
{   // reference Read.hpp:127-131 / 143-148
    double q = (1.0 - pow(10.0, -phred / 10.0));
    if (q < 0.0 || q > 1.0 || std::isnan(q) || std::isinf(q)) throw std::string("Phred error.");
    if (q < 1e-16) q = 1e-16;
    if (q > 1.0 - 1e-16) q = 1.0 - 1e-16;
    return q;
}

// reference Library.hpp:78-128
void Library::calcProb(const std::vector<double> &counts)
{
    int max_isize = 2000;
    double max_count = -1;
    for (int s = 0; s < int(counts.size()); s++)
        if (counts[size_t(s)] >= max_count) { max_count = double(int(counts[size_t(s)])); max_isize = s; }   // max_count is an int there
    maxins = 25 * max_isize;
    if (maxins > int(counts.size())) maxins = int(counts.size());
    probs.assign(size_t(maxins), 0.0);
    double z = 0.0;
    for (int d = 0; d < maxins; d++) { probs[size_t(d)] = counts[size_t(d)]; z += probs[size_t(d)]; }
    for (int d = 0; d < maxins; d++) {
        probs[size_t(d)] /= z;
        if (probs[size_t(d)] < 1e-10) probs[size_t(d)] = 1e-10;
    }
    std::vector<double> sorted(probs);
    std::sort(sorted.begin(), sorted.end());
    double sum = 0.0;
    ninetyfifth_pct_prob = sorted.empty() ? 0.0 : sorted.back();
    for (int x = int(sorted.size()) - 1; x > 0; x--) {
        sum += sorted[size_t(x)];
        if (sum > 0.95) { ninetyfifth_pct_prob = sorted[size_t(x)]; break; }
    }
}

static dd_params to_abi(const ObservationModelParameters &o)
{
    dd_params p;
    p.pError = o.pError; p.pMut = o.pMut; p.pFirstgLO = o.pFirstgLO; p.mapQualThreshold = o.mapQualThreshold;
    p.checkBaseQualThreshold = o.checkBaseQualThreshold; p.maxLengthDel = o.maxLengthDel; p.padCover = o.padCover;
    p.bMid = o.bMid; p.forceReadOnHaplotype = o.forceReadOnHaplotype ? 1 : 0; p.mapUnmappedReads = o.mapUnmappedReads ? 1 : 0;
    p.maxMismatch = o.maxMismatch;
    p.capMapQualFast = o.capMapQualFast;
    return p;
}

// Rebuilds what reportVariants derives from mapState (reference ObservationModelFB.cpp:1351-1475), from
// hpos: >=0 haplotype index, -3 LO, -4 RO, inserted base = DD_HPOS_INS_KEY0 - pos as the library writes it (pos = the x of
// the inserted state numS+x, which keys ml.indels, :1380).  A bare MLAlignment::INS (-1: an array in the reference's own
// coding) is accepted too; its key is then taken from the neighbouring entries — (previous on-haplotype base)+1 or the
// next on-haplotype base — which is what the model's transitions imply whenever the run has such a neighbour.
void LikelihoodEngine::rebuildAlignment(const Haplotype &hap, const Read &read, const int16_t *hp,
                                        const ObservationModelParameters &p, MLAlignment &ml)
{
    const int L = int(read.size()), Hs = int(hap.size());
    ml.align = std::string(Hs, 'R');
    ml.indels.clear(); ml.snps.clear(); ml.hapIndelCovered.clear(); ml.hapSNPCovered.clear();
    ml.hpos.assign(L, 0);
    ml.firstBase = -1; ml.lastBase = -1;
    ml.nBQT = 0; ml.nmmBQT = 0; ml.mLogBQ = 0.0; ml.nMMRight = 0; ml.nMMLeft = 0; ml.numIndels = 0; ml.numMismatch = 0;
    for (int b = 0; b < L; b++) ml.hpos[b] = DD_HPOS_IS_INS(hp[b]) ? int(MLAlignment::INS) : int(hp[b]);
    int b = 0;
    while (b < L) {
        const int h = hp[b];
        if (DD_HPOS_IS_INS(h)) {
            // inserted state numS+x: x-1 is the last haplotype base the read consumed before the run (an insertion
            // is entered from "on base x", ObservationModelFB.cpp:1823-1826 / 1746-1749), so pos = x (:1380)
            int rpos = b, len = 0;
            while (b < L && DD_HPOS_IS_INS(hp[b])) { b++; len++; }
            int pos;
            if (h != MLAlignment::INS) pos = DD_HPOS_INS_POS(h);  // the key the device recorded
            else if (rpos > 0 && hp[rpos - 1] >= 0) pos = hp[rpos - 1] + 1;
            else if (b < L && hp[b] >= 0) pos = hp[b];           // run starts the read: next on-haplotype base
            else pos = Hs;                                       // bare code, run followed by RO: inserted at the last base
            std::string seq = read.seq.seq.substr(rpos, len);
            ml.indels[pos] = AlignedVariant(std::string("+").append(seq), pos, pos, rpos, b - 1);
            ml.numIndels++;
            continue;
        }
        if (h >= 0) {
            if (ml.firstBase == -1) ml.firstBase = h; else if (h < ml.firstBase) ml.firstBase = h;
            if (ml.lastBase == -1) ml.lastBase = h; else if (h > ml.lastBase) ml.lastBase = h;
            if (read.qual[b] > p.checkBaseQualThreshold) {
                ml.nBQT++;
                ml.mLogBQ += log10(1.0 - read.qual[b]);
            }
            if (read.seq[b] != hap.seq[h]) {
                std::string snp;
                snp += hap.seq[h];
                snp.append("=>");
                snp += read.seq[b];
                if (read.qual[b] > p.checkBaseQualThreshold) ml.nmmBQT++;
                if (b < 6) ml.nMMLeft++;
                if (b > L - 6) ml.nMMRight++;
                if (read.qual[b] > 0.95) ml.numMismatch++;
                ml.snps[h] = AlignedVariant(snp, h, h, b, b);
                ml.align[h] = read.seq[b];
            }
            if (b < L - 1) {
                // next state on a base (or right of the haplotype) more than one position further: deletion (:1437-1453)
                const int nh = hp[b + 1];
                int ns = -1;                       // haplotype-state index (s = h+1); RO = Hs+1
                if (nh >= 0) ns = nh + 1;
                else if (nh == MLAlignment::RO) ns = Hs + 1;
                else if (nh == MLAlignment::LO) ns = 0;
                const int s = h + 1;
                if (ns >= 0 && ns - s > 1) {
                    const int pos = s;
                    const int len = ns - s - 1;
                    for (int y = pos; y < len + pos && y < Hs; y++) ml.align[y] = 'D';
                    std::string seq = hap.seq.substr(pos, len);
                    ml.indels[pos] = AlignedVariant(std::string("-").append(seq), pos, pos + len - 1, b, b + 1);
                    ml.numIndels++;
                }
            }
        }
        b++;
    }
    for (std::map<int, AlignedVariant>::const_iterator it = hap.indels.begin(); it != hap.indels.end(); ++it)
        ml.hapIndelCovered[it->first] = it->second.isCovered(p.padCover, ml.firstBase, ml.lastBase);
    for (std::map<int, AlignedVariant>::const_iterator it = hap.snps.begin(); it != hap.snps.end(); ++it)
        ml.hapSNPCovered[it->first] = it->second.isCovered(p.padCover, ml.firstBase, ml.lastBase);
}

void LikelihoodEngine::rebuildAlignmentFaster(const Haplotype &hap, const Read &read, const int16_t *hp,
                                              const ObservationModelParameters &p, MLAlignment &ml)
{
    const int L = int(read.size()), Hs = int(hap.size());
    ml.align = std::string(Hs, 'R');
    ml.indels.clear(); ml.snps.clear(); ml.hapIndelCovered.clear(); ml.hapSNPCovered.clear();
    ml.hpos.assign(size_t(L), 0);
    for (int i = 0; i < L; i++) ml.hpos[size_t(i)] = DD_HPOS_IS_INS(hp[i]) ? int(MLAlignment::INS) : int(hp[i]);
    ml.firstBase = -1; ml.lastBase = -1;
    int lhp = 1;                                       // Faster.cpp:553 (only used for a bare INS code)
    int b = 0;
    while (b < L) {
        const int h = hp[b];
        if (DD_HPOS_IS_INS(h)) {                       // Faster.cpp:606-621
            const int rpos = b;
            int len = 0;
            while (b < L && DD_HPOS_IS_INS(hp[b])) { b++; len++; }
            const int pos = (h != MLAlignment::INS) ? DD_HPOS_INS_POS(h) : lhp;   // the key the device recorded (lhp of :556-566)
            ml.indels[pos] = AlignedVariant(std::string("+").append(read.seq.seq.substr(rpos, len)), pos, pos, rpos, b - 1);
            continue;
        }
        if (h >= 0) {
            lhp = h + 1;
            if (ml.firstBase == -1) ml.firstBase = h; else if (h < ml.firstBase) ml.firstBase = h;
            if (ml.lastBase == -1) ml.lastBase = h; else if (h > ml.lastBase) ml.lastBase = h;
            if (read.seq[b] != hap.seq[h]) {           // :631-643
                std::string snp;
                snp += hap.seq[h];
                snp.append("=>");
                snp += read.seq[b];
                ml.snps[h] = AlignedVariant(snp, h, h, b, b);
                ml.align[h] = read.seq[b];
            }
            if (b < L - 1 && hp[b + 1] >= 0 && hp[b + 1] - h > 1) {     // :645-661: next state on a later base
                const int pos = h + 1, len = hp[b + 1] - h - 1;
                for (int y = pos; y < pos + len && y < Hs; y++) ml.align[y] = 'D';
                ml.indels[pos] = AlignedVariant(std::string("-").append(hap.seq.substr(pos, len)), pos, pos + len - 1, b, b + 1);
            }
        }
        b++;
    }
    for (std::map<int, AlignedVariant>::const_iterator it = hap.indels.begin(); it != hap.indels.end(); ++it)
        ml.hapIndelCovered[it->first] = it->second.isCovered(p.padCover, ml.firstBase, ml.lastBase);
    for (std::map<int, AlignedVariant>::const_iterator it = hap.snps.begin(); it != hap.snps.end(); ++it)
        ml.hapSNPCovered[it->first] = it->second.isCovered(p.padCover, ml.firstBase, ml.lastBase);
}

// ------------------------------------------------------------------------------------------------------------------------
// Flat buffers of a batch.  Result arrays are not value-initialised (4 GB of zero-fill per 10,000 windows would cost more
// than the kernels) and live in page-locked memory when the device gives it (dd_host_alloc): the D2H copies then run at
// link speed and overlap the kernels.
template <class T> struct RawBuf {
    T *p; size_t cap; bool pinned;
    RawBuf() : p(NULL), cap(0), pinned(false) {}
    ~RawBuf() { release(); }
    void release() { if (p) { if (pinned) dd_host_free(p); else free(p); } p = NULL; cap = 0; }
    T *reserve(size_t n)
    {
        if (n <= cap) return p;
        release();
        const size_t want = n + n / 8 + 64;
        p = static_cast<T *>(dd_host_alloc(want * sizeof(T)));
        pinned = p != NULL;
        if (!p) p = static_cast<T *>(malloc(want * sizeof(T)));
        if (!p) throw std::string("out of memory");
        cap = want;
        return p;
    }
    T &operator[](size_t i) { return p[i]; }
    const T &operator[](size_t i) const { return p[i]; }
private:
    RawBuf(const RawBuf &); RawBuf &operator=(const RawBuf &);
};

struct BatchBlock {
    int W;
    bool faster, has_hpos;
    ObservationModelParameters params;
    std::vector<int32_t> win_hap_off, win_read_off, hap_var_off, read_seq_off;
    std::vector<int64_t> pair_off, hpos_off, vc_off;
    RawBuf<double> ll, llOn, llOff, mLogBQ;
    RawBuf<uint8_t> offHap, offHapHMQ, vcov, fcov;
    RawBuf<int16_t> numIndels, numMismatch, nBQT, nmmBQT, nMMLeft, nMMRight, firstBase, lastBase, hpos;
    RawBuf<int32_t> status;
    bool has_cigars; int cig_cap;                        // device CIGARs (setDeviceCigars): per pair, ops at pair * cig_cap
    RawBuf<int32_t> cig_n_ops, cig_ref_off, cig_status;
    RawBuf<uint32_t> cig_ops;
    bool has_realign;                                    // device realign (setDeviceRealign): per READ, ops at read * cig_cap
    RawBuf<int32_t> rl_hap, rl_status, rl_n_ops, rl_ref_off;
    RawBuf<uint32_t> rl_ops;
    RawBuf<uint8_t> on_hap;                              // ... and the device's onHap, which its rule consults
    bool has_pairs;                                      // device pair (setDeviceRealignDiploid): per WINDOW; the realign rows are then the diploid rule's
    RawBuf<int32_t> dp_pair, dp_state;
    RawBuf<double> dp_best, dp_gap, dp_margin;
    bool has_keys;                                       // device indel keys (setDeviceIndelKeys): per pair, the --faster model
    RawBuf<int16_t> indel_keys;
    int device; bool long_faster, wide;                  // ... and what a recomputation of one of its windows needs of the engine that made it
    BatchBlock() : W(0), faster(false), has_hpos(false), has_cigars(false), cig_cap(0), has_realign(false), has_pairs(false), has_keys(false),
                   device(0), long_faster(false), wide(false) {}
};

struct PackScratch {
    std::vector<int32_t> hap_seq_off, hap_var, hap_var_flank;
    std::vector<uint32_t> win_hap_start, read_start;
    std::vector<char> hap_seq;
    RawBuf<char> read_seq;               // the two big inputs (one byte per read base each) sit in page-locked memory: their
    RawBuf<uint8_t> read_qidx;           // H2D copy then runs at link speed instead of through the driver's staging buffers
    std::vector<uint8_t> read_mqidx, read_flags, read_lib;
    std::vector<int32_t> read_mate_pos, read_mate_len;
    std::vector<double> pair_prior;      // device pair: the jobs' prior tables, one after the other
    std::vector<int32_t> hap_n_indels;   // ... and Haplotype::countIndels per haplotype
    std::vector<int32_t> hap_ref_pos;    // device CIGARs: Haplotype::refHpos per haplotype base
    std::vector<uint8_t> hap_aligned;    // ... and whether the haplotype has one
};

namespace {

// value -> small index, shared by the packing threads: a lock-free read of the per-thread cache, the shared table under a mutex
// on a miss (at most 256 distinct values per batch: BAM qualities are integer Phred)
class ValueTable {
public:
    std::vector<double> tab;
    int intern(double v)
    {
        std::lock_guard<std::mutex> g(m_);
        for (size_t i = 0; i < tab.size(); i++)
            if (memcmp(&tab[i], &v, sizeof(double)) == 0) return int(i);
        if (tab.size() >= 256) return -1;
        tab.push_back(v);
        return int(tab.size()) - 1;
    }
private:
    std::mutex m_;
};

struct ValueCache {                      // per thread: open addressing on the bit pattern
    uint64_t key[512]; int16_t val[512];
    ValueCache() { for (int i = 0; i < 512; i++) val[i] = -1; }
    int get(double v, ValueTable &T)
    {
        uint64_t k;
        memcpy(&k, &v, 8);
        unsigned h = unsigned((k * 0x9E3779B97F4A7C15ull) >> 55);
        for (;;) {
            if (val[h] < 0) {
                const int idx = T.intern(v);
                if (idx < 0) return -1;
                key[h] = k; val[h] = int16_t(idx);
                return idx;
            }
            if (key[h] == k) return val[h];
            h = (h + 1) & 511;
        }
    }
};

unsigned pick_threads(int hostThreads, int64_t units)
{
    unsigned nthr = std::thread::hardware_concurrency();
    if (nthr > 16) nthr = 16;
    if (nthr < 1) nthr = 1;
    if (hostThreads > 0) nthr = unsigned(hostThreads);
    if (int64_t(nthr) > units) nthr = unsigned(units > 0 ? units : 1);
    return nthr;
}

template <class F> void parallel_windows(int W, unsigned nthr, int grain, F f)
{
    if (nthr <= 1 || W <= grain) { for (int w = 0; w < W; w++) f(w); return; }
    std::atomic<int> next(0);
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nthr; t++)
        pool.push_back(std::thread([&]() {
            for (int w0 = next.fetch_add(grain); w0 < W; w0 = next.fetch_add(grain))
                for (int w = w0; w < W && w < w0 + grain; w++) f(w);
        }));
    for (size_t t = 0; t < pool.size(); t++) pool[t].join();
}

// one record from the block (what the reference's loop body leaves in liks[h][r], DInDel.cpp:1717-1719)
void fill_record(const BatchBlock &B, int w, size_t h, size_t r, const Haplotype &Hh, const Read &Rd, MLAlignment &ml)
{
    const size_t Rn = size_t(B.win_read_off[w + 1] - B.win_read_off[w]);
    const int r0 = B.win_read_off[w];
    const int g = B.win_hap_off[w] + int(h);
    const int nv = B.hap_var_off[g + 1] - B.hap_var_off[g];
    const int64_t p = B.pair_off[w] + int64_t(h) * int64_t(Rn) + int64_t(r);
    const int64_t SL = int64_t(B.read_seq_off[B.win_read_off[w + 1]]) - B.read_seq_off[r0];
    const int L = int(Rd.size()), Hs = int(Hh.size());
    const int16_t *hp = B.hpos.p + B.hpos_off[w] + int64_t(h) * SL + (B.read_seq_off[r0 + r] - B.read_seq_off[r0]);
    const int64_t vb = B.vc_off[w] + int64_t(B.hap_var_off[g] - B.hap_var_off[B.win_hap_off[w]]) * int64_t(Rn) + int64_t(r) * nv;
    // Per pair the device already delivers every counter of the record; the variant maps and the `align` string need the
    // per-base walk (rebuildAlignment) only when the read shows an indel or differs from the haplotype segment it sits on.
    bool plain = false;                       // gap-free, mismatch-free placement: nothing to list
    if (!B.faster && B.numIndels[p] == 0) {
        if (B.firstBase[p] < 0) plain = true;   // no base on the haplotype
        else {
            int b0 = 0;
            while (b0 < L && hp[b0] < 0) b0++;
            const int n = B.lastBase[p] - B.firstBase[p] + 1;
            plain = b0 + n <= L && hp[b0] == B.firstBase[p] &&
                    memcmp(Rd.seq.seq.data() + b0, Hh.seq.data() + B.firstBase[p], size_t(n)) == 0;
        }
    }
    if (plain) {
        ml.align = std::string(size_t(Hs), 'R');
        ml.indels.clear(); ml.snps.clear(); ml.hapIndelCovered.clear(); ml.hapSNPCovered.clear();
        ml.hpos.assign(hp, hp + L);              // no inserted base in a plain placement: the codes are the reference's
        ml.firstBase = B.firstBase[p]; ml.lastBase = B.lastBase[p];
        ml.numIndels = 0; ml.numMismatch = B.numMismatch[p]; ml.nBQT = B.nBQT[p]; ml.nmmBQT = B.nmmBQT[p];
        ml.nMMLeft = B.nMMLeft[p]; ml.nMMRight = B.nMMRight[p];
        int i = 0;
        for (std::map<int, AlignedVariant>::const_iterator it = Hh.indels.begin(); it != Hh.indels.end(); ++it, ++i)
            ml.hapIndelCovered[it->first] = B.vcov[vb + i] != 0;
        for (std::map<int, AlignedVariant>::const_iterator it = Hh.snps.begin(); it != Hh.snps.end(); ++it, ++i)
            ml.hapSNPCovered[it->first] = B.vcov[vb + i] != 0;
    } else if (B.faster) LikelihoodEngine::rebuildAlignmentFaster(Hh, Rd, hp, B.params, ml);
    else LikelihoodEngine::rebuildAlignment(Hh, Rd, hp, B.params, ml);
    ml.ll = B.ll[p]; ml.llOn = B.llOn[p]; ml.llOff = B.llOff[p];
    ml.offHap = B.offHap[p] != 0; ml.offHapHMQ = B.offHapHMQ[p] != 0;
    if (!B.faster) ml.mLogBQ = B.mLogBQ[p];           // the device's serial sum (same order as the reference)
    ml.hapIndelFilterCovered.clear();
    {   // per haplotype-indel coverage flags of filterHaplotypes, in hap.indels map order (first nvI of the hap's list)
        int i = 0;
        for (std::map<int, AlignedVariant>::const_iterator it = Hh.indels.begin(); it != Hh.indels.end(); ++it, ++i)
            ml.hapIndelFilterCovered[it->first] = B.fcov[vb + i] != 0;
    }
}

} // namespace

// ---------------- WindowLikelihoods: the lazy view ----------------
size_t WindowLikelihoods::numHaps() const { return size_t(blk_->win_hap_off[w_ + 1] - blk_->win_hap_off[w_]); }
size_t WindowLikelihoods::numReads() const { return size_t(blk_->win_read_off[w_ + 1] - blk_->win_read_off[w_]); }
int64_t WindowLikelihoods::pair(size_t h, size_t r) const { return blk_->pair_off[w_] + int64_t(h) * int64_t(numReads()) + int64_t(r); }
double WindowLikelihoods::ll(size_t h, size_t r) const { return blk_->ll[pair(h, r)]; }
double WindowLikelihoods::llOn(size_t h, size_t r) const { return blk_->llOn[pair(h, r)]; }
double WindowLikelihoods::llOff(size_t h, size_t r) const { return blk_->llOff[pair(h, r)]; }
double WindowLikelihoods::mLogBQ(size_t h, size_t r) const { return blk_->mLogBQ[pair(h, r)]; }
bool WindowLikelihoods::offHap(size_t h, size_t r) const { return blk_->offHap[pair(h, r)] != 0; }
bool WindowLikelihoods::offHapHMQ(size_t h, size_t r) const { return blk_->offHapHMQ[pair(h, r)] != 0; }
int WindowLikelihoods::numIndels(size_t h, size_t r) const { return blk_->numIndels[pair(h, r)]; }
bool WindowLikelihoods::hasDeviceCigars() const { return blk_ && blk_->has_cigars; }
int WindowLikelihoods::cigarOpsCap() const { return blk_->cig_cap; }
int WindowLikelihoods::cigarStatus(size_t h, size_t r) const { return blk_->cig_status[pair(h, r)]; }
int WindowLikelihoods::cigarNumOps(size_t h, size_t r) const { return blk_->cig_n_ops[pair(h, r)]; }
const uint32_t *WindowLikelihoods::cigarOps(size_t h, size_t r) const { return blk_->cig_ops.p + size_t(pair(h, r)) * size_t(blk_->cig_cap); }
int WindowLikelihoods::cigarRefOff(size_t h, size_t r) const { return blk_->cig_ref_off[pair(h, r)]; }
bool WindowLikelihoods::hasDeviceRealign() const { return blk_ && blk_->has_realign; }
int WindowLikelihoods::realignHap(size_t r) const { return blk_->rl_hap[size_t(blk_->win_read_off[w_]) + r]; }
int WindowLikelihoods::realignStatus(size_t r) const { return blk_->rl_status[size_t(blk_->win_read_off[w_]) + r]; }
int WindowLikelihoods::realignNumOps(size_t r) const { return blk_->rl_n_ops[size_t(blk_->win_read_off[w_]) + r]; }
const uint32_t *WindowLikelihoods::realignOps(size_t r) const { return blk_->rl_ops.p + (size_t(blk_->win_read_off[w_]) + r) * size_t(blk_->cig_cap); }
int WindowLikelihoods::realignRefOff(size_t r) const { return blk_->rl_ref_off[size_t(blk_->win_read_off[w_]) + r]; }
bool WindowLikelihoods::hasDevicePair() const { return blk_ && blk_->has_pairs; }
int WindowLikelihoods::pairState() const { return blk_->dp_state[size_t(w_)]; }
std::pair<int, int> WindowLikelihoods::devicePair() const { return std::pair<int, int>(blk_->dp_pair[2 * size_t(w_)], blk_->dp_pair[2 * size_t(w_) + 1]); }

WindowLikelihoods WindowLikelihoods::handMadeRealign(const std::vector<Haplotype> &haps, const std::vector<Read> &reads, int opsCap, const int32_t *hap,
                                                     const int32_t *status, const int32_t *nOps, const uint32_t *ops, const int32_t *refOff,
                                                     const int16_t *hpos, const double *ll, int pairState, const int32_t *pair)
{
    std::shared_ptr<BatchBlock> blk = std::make_shared<BatchBlock>();
    BatchBlock &B = *blk;
    const size_t H = haps.size(), Rn = reads.size(), np = H * Rn + 1, cap = size_t(opsCap < 1 ? 1 : opsCap);
    B.W = 1; B.has_realign = hap != NULL; B.cig_cap = int(cap); B.has_hpos = hpos != NULL;
    B.win_hap_off.assign(2, 0); B.win_hap_off[1] = int32_t(H);
    B.win_read_off.assign(2, 0); B.win_read_off[1] = int32_t(Rn);
    B.hap_var_off.assign(H + 1, 0);
    B.read_seq_off.assign(Rn + 1, 0);
    for (size_t r = 0; r < Rn; r++) B.read_seq_off[r + 1] = B.read_seq_off[r] + int32_t(reads[r].size());
    const size_t SL = size_t(B.read_seq_off[Rn]);
    B.pair_off.assign(2, 0); B.pair_off[1] = int64_t(H * Rn);
    B.hpos_off.assign(2, 0); B.hpos_off[1] = int64_t(H * SL);
    B.vc_off.assign(2, 0);
    // every pair a plain placement without a base on the haplotype: get() then hands the given hpos through as it is
    B.ll.reserve(np); B.llOn.reserve(np); B.llOff.reserve(np); B.mLogBQ.reserve(np); B.offHap.reserve(np); B.offHapHMQ.reserve(np);
    B.status.reserve(np); B.numIndels.reserve(np); B.numMismatch.reserve(np); B.nBQT.reserve(np); B.nmmBQT.reserve(np);
    B.nMMLeft.reserve(np); B.nMMRight.reserve(np); B.firstBase.reserve(np); B.lastBase.reserve(np); B.vcov.reserve(1); B.fcov.reserve(1);
    for (size_t p = 0; p < np; p++) {
        B.ll[p] = B.llOn[p] = B.llOff[p] = B.mLogBQ[p] = 0.0; B.offHap[p] = B.offHapHMQ[p] = 0; B.status[p] = DD_PAIR_OK;
        B.numIndels[p] = B.numMismatch[p] = B.nBQT[p] = B.nmmBQT[p] = B.nMMLeft[p] = B.nMMRight[p] = 0; B.firstBase[p] = B.lastBase[p] = -1;
    }
    if (ll) memcpy(B.ll.p, ll, H * Rn * sizeof(double));
    if (pairState >= 0) {
        B.has_pairs = true;
        B.dp_pair.reserve(2); B.dp_state.reserve(1); B.dp_best.reserve(1); B.dp_gap.reserve(1); B.dp_margin.reserve(1);
        B.dp_state[0] = pairState; B.dp_pair[0] = pair ? pair[0] : -1; B.dp_pair[1] = pair ? pair[1] : -1;
        B.dp_best[0] = B.dp_gap[0] = B.dp_margin[0] = 0.0;
    }
    if (hpos) { B.hpos.reserve(H * SL + 1); memcpy(B.hpos.p, hpos, H * SL * sizeof(int16_t)); }
    if (hap) {
        B.rl_hap.reserve(Rn + 1); B.rl_status.reserve(Rn + 1); B.rl_n_ops.reserve(Rn + 1); B.rl_ref_off.reserve(Rn + 1); B.rl_ops.reserve(Rn * cap + 1);
        memcpy(B.rl_hap.p, hap, Rn * 4); memcpy(B.rl_status.p, status, Rn * 4); memcpy(B.rl_n_ops.p, nOps, Rn * 4);
        memcpy(B.rl_ref_off.p, refOff, Rn * 4); memcpy(B.rl_ops.p, ops, Rn * cap * 4);
    }
    WindowLikelihoods v;
    v.blk_ = blk; v.w_ = 0; v.haps_ = &haps; v.reads_ = &reads;
    return v;
}

WindowLikelihoods WindowLikelihoods::handMadeFaster(const std::vector<Haplotype> &haps, const std::vector<Read> &reads, const int16_t *hpos,
                                                    const int16_t *keys, LikelihoodEngine *eng)
{
    WindowLikelihoods v = handMadeRealign(haps, reads, 1, NULL, NULL, NULL, NULL, NULL, hpos);
    BatchBlock &B = const_cast<BatchBlock &>(*v.blk_);     // (just made, nobody else refers to it)
    B.faster = true;
    if (eng) { B.params = eng->params; B.device = eng->device_; B.long_faster = eng->longWindowsFaster_; B.wide = eng->wideDeletions_; }
    if (keys) {
        const size_t np = haps.size() * reads.size();
        B.has_keys = true;
        B.indel_keys.reserve(np + 1);
        memcpy(B.indel_keys.p, keys, np * sizeof(int16_t));
    }
    v.eng_ = eng;
    return v;
}

static std::atomic<long> g_indel_key_fallbacks(0);
long LikelihoodEngine::indelKeyFallbacks() { return g_indel_key_fallbacks.load(); }
bool WindowLikelihoods::hasDeviceIndelKeys() const { return blk_ && blk_->has_keys; }
int WindowLikelihoods::deviceIndelKeys(size_t h, size_t r) const { return blk_->indel_keys[pair(h, r)]; }

int WindowLikelihoods::indelCount(size_t h, size_t r) const
{
    const BatchBlock &B = *blk_;
    if (!B.faster) return B.numIndels[pair(h, r)];
    if (B.has_keys) {                      // the device walked hpos (csrc/indel_keys_kernel.h); more than 64 keys: the record, as below
        const int v = B.indel_keys[pair(h, r)];
        if (v >= 0) return v;
        // The recompute-with-alignments path of get(), with an engine of its own: indelCount is called from reduce threads while the
        // engine that made the block packs its next batch (or is gone), so that engine is not touched.
        g_indel_key_fallbacks.fetch_add(1);
        if (!full_) {
            LikelihoodEngine own(B.params, B.device);
            own.setLongWindowsFaster(B.long_faster);
            own.setWideDeletions(B.wide);
            std::vector<WindowJob> one(1);
            one[0].haps = haps_; one[0].reads = reads_; one[0].leftPos = leftPos_; one[0].rightPos = leftPos_ + 1;
            own.runBatch(one, true);
            if (!one[0].error.empty()) throw one[0].error;
            full_ = one[0].result.blk_;
        }
        MLAlignment ml;
        fill_record(*full_, 0, h, r, (*haps_)[h], (*reads_)[r], ml);
        return int(ml.indels.size());
    }
    if (!B.has_hpos) return int(get(h, r).indels.size());
    // --faster: the size of the record's indel map needs the walk over hpos (rebuildAlignmentFaster), but not the record:
    // the keys that walk would enter — an insertion run's recorded position, a deletion's first base — counted once each
    const int r0 = B.win_read_off[w_];
    const int64_t SL = int64_t(B.read_seq_off[B.win_read_off[w_ + 1]]) - B.read_seq_off[r0];
    const int16_t *hp = B.hpos.p + B.hpos_off[w_] + int64_t(h) * SL + (B.read_seq_off[size_t(r0) + r] - B.read_seq_off[r0]);
    const int L = int((*reads_)[r].size());
    int keys[64], nk = 0, lhp = 1, b = 0;
    bool spilled = false;
    while (b < L && !spilled) {
        const int c = hp[b];
        int key = -1;
        if (DD_HPOS_IS_INS(c)) {
            while (b < L && DD_HPOS_IS_INS(hp[b])) b++;
            key = (c != MLAlignment::INS) ? DD_HPOS_INS_POS(c) : lhp;
        } else {
            if (c >= 0) { lhp = c + 1; if (b < L - 1 && hp[b + 1] >= 0 && hp[b + 1] - c > 1) key = c + 1; }
            b++;
        }
        if (key >= 0) {
            bool seen = false;
            for (int k = 0; k < nk; k++) if (keys[k] == key) seen = true;
            if (!seen) { if (nk == 64) spilled = true; else keys[nk++] = key; }
        }
    }
    return spilled ? int(get(h, r).indels.size()) : nk;
}
int WindowLikelihoods::numMismatch(size_t h, size_t r) const { return blk_->numMismatch[pair(h, r)]; }
int WindowLikelihoods::nBQT(size_t h, size_t r) const { return blk_->nBQT[pair(h, r)]; }
int WindowLikelihoods::nmmBQT(size_t h, size_t r) const { return blk_->nmmBQT[pair(h, r)]; }
int WindowLikelihoods::nMMLeft(size_t h, size_t r) const { return blk_->nMMLeft[pair(h, r)]; }
int WindowLikelihoods::nMMRight(size_t h, size_t r) const { return blk_->nMMRight[pair(h, r)]; }
int WindowLikelihoods::firstBase(size_t h, size_t r) const { return blk_->firstBase[pair(h, r)]; }
int WindowLikelihoods::lastBase(size_t h, size_t r) const { return blk_->lastBase[pair(h, r)]; }
// onHap[r] = 1 if the read lies on some haplotype under the artificial mapping quality (DInDel.cpp:1720: !liks[hidx][r].offHapHMQ for any hidx).
// Taken from the offHapHMQ flags here instead of from the device's dd_onhap_kernel: one kernel (and one kernel boundary, ~0.15 ms on
// this part) less per batch, for a value only the realigned-BAM step reads.
int WindowLikelihoods::onHap(size_t r) const
{
    const size_t nh = numHaps();
    for (size_t h = 0; h < nh; h++) if (!blk_->offHapHMQ[pair(h, r)]) return 1;
    return 0;
}

// slot of the haplotype's variant `key` in the per-pair flag list: hap.indels in map order, then hap.snps (-1: no such variant)
int WindowLikelihoods::varSlot(size_t h, int key, bool snp) const
{
    const Haplotype &H = (*haps_)[h];
    const std::map<int, AlignedVariant> &m = snp ? H.snps : H.indels;
    std::map<int, AlignedVariant>::const_iterator it = m.find(key);
    if (it == m.end()) return -1;
    return int(std::distance(m.begin(), it)) + (snp ? int(H.indels.size()) : 0);
}

static inline int64_t var_base(const BatchBlock &B, int w, size_t h, size_t r)
{
    const int g = B.win_hap_off[w] + int(h);
    const int64_t Rn = B.win_read_off[w + 1] - B.win_read_off[w];
    return B.vc_off[w] + int64_t(B.hap_var_off[g] - B.hap_var_off[B.win_hap_off[w]]) * Rn + int64_t(r) * (B.hap_var_off[g + 1] - B.hap_var_off[g]);
}

bool WindowLikelihoods::hapIndelCovered(size_t h, size_t r, int key) const
{
    const int s = varSlot(h, key, false);
    return s >= 0 && blk_->vcov[var_base(*blk_, w_, h, r) + s] != 0;
}
bool WindowLikelihoods::hapSNPCovered(size_t h, size_t r, int key) const
{
    const int s = varSlot(h, key, true);
    return s >= 0 && blk_->vcov[var_base(*blk_, w_, h, r) + s] != 0;
}
bool WindowLikelihoods::hapIndelFilterCovered(size_t h, size_t r, int key) const
{
    const int s = varSlot(h, key, false);
    return s >= 0 && blk_->fcov[var_base(*blk_, w_, h, r) + s] != 0;
}

bool WindowLikelihoods::coveredAt(size_t h, size_t r, int slot) const { return slot >= 0 && blk_->vcov[var_base(*blk_, w_, h, r) + slot] != 0; }
bool WindowLikelihoods::filterCoveredAt(size_t h, size_t r, int slot) const { return slot >= 0 && blk_->fcov[var_base(*blk_, w_, h, r) + slot] != 0; }

WindowLikelihoods::Rows WindowLikelihoods::rows(size_t h) const
{
    const BatchBlock &B = *blk_;
    const int64_t p = pair(h, 0);
    const int g = B.win_hap_off[w_] + int(h);
    Rows R;
    R.ll = B.ll.p + p; R.llOn = B.llOn.p + p; R.llOff = B.llOff.p + p; R.mLogBQ = B.mLogBQ.p + p;
    R.offHap = B.offHap.p + p; R.offHapHMQ = B.offHapHMQ.p + p;
    R.numIndels = B.numIndels.p + p; R.numMismatch = B.numMismatch.p + p; R.nBQT = B.nBQT.p + p; R.nmmBQT = B.nmmBQT.p + p;
    R.nMMLeft = B.nMMLeft.p + p; R.nMMRight = B.nMMRight.p + p; R.firstBase = B.firstBase.p + p; R.lastBase = B.lastBase.p + p;
    R.nv = B.hap_var_off[g + 1] - B.hap_var_off[g];
    const int64_t vb = var_base(B, w_, h, 0);
    R.vcov = B.vcov.p + vb; R.fcov = B.fcov.p + vb;
    return R;
}

MLAlignment WindowLikelihoods::get(size_t h, size_t r) const
{
    MLAlignment ml;
    if (blk_->has_hpos) { fill_record(*blk_, w_, h, r, (*haps_)[h], (*reads_)[r], ml); return ml; }
    if (!full_) {                          // the batch kept no alignments: this window once more, with them
        if (!eng_) throw std::string("WindowLikelihoods::get: batch was run without alignments and the engine is gone");
        std::vector<WindowJob> one(1);
        one[0].haps = haps_; one[0].reads = reads_; one[0].leftPos = leftPos_; one[0].rightPos = leftPos_ + 1;
        const bool keep = eng_->keepAlignments_, cig = eng_->deviceCigars_, rl = eng_->deviceRealign_, dip = eng_->deviceRealignDiploid_;
        const bool ik = eng_->deviceIndelKeys_;
        eng_->keepAlignments_ = true; eng_->deviceCigars_ = false; eng_->deviceRealign_ = false; eng_->deviceRealignDiploid_ = false;
        eng_->deviceIndelKeys_ = false;
        try { eng_->runBatch(one, blk_->faster); }
        catch (...) { eng_->keepAlignments_ = keep; eng_->deviceCigars_ = cig; eng_->deviceRealign_ = rl; eng_->deviceRealignDiploid_ = dip; eng_->deviceIndelKeys_ = ik; throw; }
        eng_->keepAlignments_ = keep; eng_->deviceCigars_ = cig; eng_->deviceRealign_ = rl; eng_->deviceRealignDiploid_ = dip; eng_->deviceIndelKeys_ = ik;
        if (!one[0].error.empty()) throw one[0].error;
        full_ = one[0].result.blk_;
    }
    fill_record(*full_, 0, h, r, (*haps_)[h], (*reads_)[r], ml);
    return ml;
}

void WindowLikelihoods::toLiks(std::vector<std::vector<MLAlignment> > &liks, std::vector<int> &onHapV) const
{
    const size_t H = numHaps(), Rn = numReads();
    onHapV = std::vector<int>(Rn, 0);
    liks = std::vector<std::vector<MLAlignment> >(H, std::vector<MLAlignment>(Rn));
    for (size_t h = 0; h < H; h++)
        for (size_t r = 0; r < Rn; r++) liks[h][r] = get(h, r);
    for (size_t r = 0; r < Rn; r++) onHapV[r] = onHap(r);
}

// ---------------- LikelihoodEngine ----------------
void LikelihoodEngine::computeLikelihoodsFaster(const std::vector<Haplotype> &haps, const std::vector<Read> &reads,
                                                std::vector<std::vector<MLAlignment> > &liks, uint32_t leftPos,
                                                uint32_t rightPos, std::vector<int> &onHap)
{
    std::vector<WindowJob> jobs(1);
    jobs[0].haps = &haps; jobs[0].reads = &reads; jobs[0].leftPos = leftPos; jobs[0].rightPos = rightPos;
    jobs[0].liks = &liks; jobs[0].onHap = &onHap;
    runBatch(jobs, true);
    if (!jobs[0].error.empty()) throw jobs[0].error;
}

void LikelihoodEngine::warmUp(size_t pairs)
{
    // per pair: ~25 input bytes (a read of 100 bases is shared by its window's haplotypes) and ~270 result bytes if everything is staged
    const size_t bytes = pairs * 300 + (size_t(32) << 20);
    if (dd_reserve_cache(device_, bytes, bytes <= (size_t(64) << 20) ? bytes : 0) != DD_SUCCESS) throw std::string("dd_reserve_cache: ") + dd_last_error();
    // two result blocks with their per-pair arrays at that size, made now (page-locking 90 MB takes 40-100 ms): a pipelined caller
    // would otherwise grow its blocks step by step under its first batches.  The per-base and per-variant arrays follow the data.
    const size_t np = pairs + 1;
    while (spare_.size() < 2) {
        std::shared_ptr<BatchBlock> blk = std::make_shared<BatchBlock>();
        BatchBlock &B = *blk;
        B.ll.reserve(np); B.llOn.reserve(np); B.llOff.reserve(np); B.mLogBQ.reserve(np);
        B.offHap.reserve(np); B.offHapHMQ.reserve(np); B.status.reserve(np);
        B.numIndels.reserve(np); B.numMismatch.reserve(np); B.nBQT.reserve(np); B.nmmBQT.reserve(np);
        B.nMMLeft.reserve(np); B.nMMRight.reserve(np); B.firstBase.reserve(np); B.lastBase.reserve(np);
        spare_.push_back(blk);
    }
}

void LikelihoodEngine::computeLikelihoodsFasterBatch(std::vector<WindowJob> &jobs) { runBatch(jobs, true); }

void LikelihoodEngine::computeLikelihoodsBatch(std::vector<WindowJob> &jobs) { runBatch(jobs, false); }

void LikelihoodEngine::computeLikelihoods(const std::vector<Haplotype> &haps, const std::vector<Read> &reads,
                                          std::vector<std::vector<MLAlignment> > &liks, uint32_t leftPos,
                                          uint32_t rightPos, std::vector<int> &onHap)
{
    std::vector<WindowJob> jobs(1);
    jobs[0].haps = &haps; jobs[0].reads = &reads; jobs[0].leftPos = leftPos; jobs[0].rightPos = rightPos;
    jobs[0].liks = &liks; jobs[0].onHap = &onHap;
    computeLikelihoodsBatch(jobs);
    if (!jobs[0].error.empty()) throw jobs[0].error;
}

void LikelihoodEngine::runBatch(std::vector<WindowJob> &jobs, bool faster)
{
    const std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
    const int W = int(jobs.size());
    // The result block of an earlier call is reused when no view refers to it any more (its pages are mapped and, when
    // pinned, registered with the device already); otherwise a new one is made and the old one lives on with its views.
    for (int w = 0; w < W; w++) jobs[w].result = WindowLikelihoods();      // views of an earlier call held by these jobs
    // A pipelined caller (dindel_gpu: batch k+1 computes while batch k reduces) keeps two or three blocks alive in turn,
    // so a few are remembered.
    std::shared_ptr<BatchBlock> blk;
    for (size_t i = 0; i < spare_.size() && !blk; i++) if (spare_[i].use_count() == 1) blk = spare_[i];
    if (!blk) {
        blk = std::make_shared<BatchBlock>();
        if (spare_.size() < 4) spare_.push_back(blk);
        else spare_[size_t(spareNext_++ % 4)] = blk;
    }
    if (!scratch_) scratch_ = std::make_shared<PackScratch>();
    BatchBlock &B = *blk;
    PackScratch &S = *scratch_;
    B.W = W; B.faster = faster; B.params = params; B.device = device_; B.long_faster = longWindowsFaster_; B.wide = wideDeletions_;
    bool any_eager = false;
    for (int w = 0; w < W; w++) if (jobs[w].liks) any_eager = true;
    // device CIGARs: the pairs' CIGARs come back instead of their alignments (main model, lazy jobs only)
    // device realign: the reads' chosen haplotypes and CIGARs come back instead of either (main model, lazy jobs only)
    // device pair: the diploid step's realigned reads — the windows' pairs chosen and certified on the device, then the rows of device realign
    B.has_pairs = deviceRealignDiploid_ && !faster && !any_eager;
    B.has_realign = (deviceRealign_ || deviceRealignDiploid_) && !faster && !any_eager;
    B.has_cigars = deviceCigars_ && !faster && !any_eager && !B.has_realign;
    B.cig_cap = cigarOpsCap_;
    // device indel keys: the pairs' indel-map key counts come back instead of their alignments (--faster model, lazy jobs only)
    B.has_keys = deviceIndelKeys_ && faster && !any_eager;
    B.has_hpos = !B.has_cigars && !B.has_realign && !B.has_keys && (keepAlignments_ || any_eager);
    const bool pack_ref_pos = B.has_cigars || B.has_realign;

    // ---- pack (CSR), pass 1: sizes and offsets.  Per window in parallel (its haplotypes and reads are scattered objects: the pass is
    // cache misses), one serial prefix sum over the windows in between ----
    const bool with_mates = params.mapUnmappedReads && !faster;
    const unsigned nthr1 = pick_threads(hostThreads_, W);
    std::vector<int64_t> whb(size_t(W) + 1, 0), wrb(size_t(W) + 1, 0), wvar(size_t(W) + 1, 0);       // per window: haplotype bases, read bases, variants
    B.win_hap_off.assign(size_t(W) + 1, 0); B.win_read_off.assign(size_t(W) + 1, 0);
    std::atomic<int> bad_read(0);
    parallel_windows(W, nthr1, 16, [&](int w) {
        WindowJob &J = jobs[w];
        J.error.clear();
        int64_t hb = 0, rb = 0, nv = 0;
        for (size_t h = 0; h < J.haps->size(); h++) { const Haplotype &H = (*J.haps)[h]; hb += int64_t(H.seq.size()); nv += int64_t(H.indels.size() + H.snps.size()); }
        for (size_t r = 0; r < J.reads->size(); r++) {
            const Read &R = (*J.reads)[r];
            if (R.qual.size() != R.size()) bad_read.store(1);
            rb += int64_t(R.size());
        }
        whb[size_t(w) + 1] = hb; wrb[size_t(w) + 1] = rb; wvar[size_t(w) + 1] = nv;
        B.win_hap_off[size_t(w) + 1] = int32_t(J.haps->size()); B.win_read_off[size_t(w) + 1] = int32_t(J.reads->size());
    });
    if (bad_read.load()) throw std::string("Read: qual and seq differ in length");
    for (int w = 0; w < W; w++) {
        whb[size_t(w) + 1] += whb[size_t(w)]; wrb[size_t(w) + 1] += wrb[size_t(w)]; wvar[size_t(w) + 1] += wvar[size_t(w)];
        B.win_hap_off[size_t(w) + 1] += B.win_hap_off[size_t(w)]; B.win_read_off[size_t(w) + 1] += B.win_read_off[size_t(w)];
        if (whb[size_t(w) + 1] > 0x7fffffffLL || wrb[size_t(w) + 1] > 0x7fffffffLL)
            throw std::string("batch too large: more than 2^31 haplotype or read bases (split the windows over several calls)");
    }
    const int64_t n_hap_bases = whb[size_t(W)], n_read_bases = wrb[size_t(W)];
    B.hap_var_off.resize(size_t(B.win_hap_off[size_t(W)]) + 1); S.hap_seq_off.resize(size_t(B.win_hap_off[size_t(W)]) + 1);
    B.read_seq_off.resize(size_t(B.win_read_off[size_t(W)]) + 1);
    B.hap_var_off[0] = 0; S.hap_seq_off[0] = 0; B.read_seq_off[0] = 0;
    parallel_windows(W, nthr1, 16, [&](int w) {
        const WindowJob &J = jobs[w];
        int64_t hb = whb[size_t(w)], rb = wrb[size_t(w)], nv = wvar[size_t(w)];
        const size_t g0 = size_t(B.win_hap_off[size_t(w)]), q0 = size_t(B.win_read_off[size_t(w)]);
        for (size_t h = 0; h < J.haps->size(); h++) {
            const Haplotype &H = (*J.haps)[h];
            hb += int64_t(H.seq.size()); nv += int64_t(H.indels.size() + H.snps.size());
            S.hap_seq_off[g0 + h + 1] = int32_t(hb);
            B.hap_var_off[g0 + h + 1] = int32_t(nv);
        }
        for (size_t r = 0; r < J.reads->size(); r++) { rb += int64_t((*J.reads)[r].size()); B.read_seq_off[q0 + r + 1] = int32_t(rb); }
    });
    std::vector<int32_t> lib_off(1, 0);
    std::vector<double> lib_prob, lib_p95;
    if (with_mates) {                                    // libraries in order of first appearance (serial: the order defines the indices)
        std::map<const Library *, int> lib_index;
        S.read_lib.clear();
        for (int w = 0; w < W; w++) {
            const WindowJob &J = jobs[w];
            for (size_t r = 0; r < J.reads->size(); r++) {
                const Read &R = (*J.reads)[r];
                int li = 0;
                if (R.isPaired()) {                      // the reference dereferences the library of paired reads only (:279-289)
                    if (!R.library) throw std::string("Cannot find library: ");            // Read.hpp:176
                    std::map<const Library *, int>::iterator lt = lib_index.find(R.library);
                    if (lt == lib_index.end()) {
                        if (lib_index.size() >= 256) throw std::string("more than 256 libraries in one batch");
                        lt = lib_index.insert(std::make_pair(R.library, int(lib_index.size()))).first;
                        lib_prob.insert(lib_prob.end(), R.library->table().begin(), R.library->table().end());
                        lib_off.push_back(int32_t(lib_prob.size()));
                        lib_p95.push_back(R.library->getNinetyFifthPctProb());
                    }
                    li = lt->second;
                }
                S.read_lib.push_back(uint8_t(li));
            }
        }
    }
    const size_t n_haps = size_t(B.win_hap_off[W]), n_reads = size_t(B.win_read_off[W]), n_var = size_t(B.hap_var_off[n_haps]);
    S.win_hap_start.resize(size_t(W)); S.hap_seq.resize(size_t(n_hap_bases) + 1); S.read_seq.reserve(size_t(n_read_bases) + 1);
    S.read_qidx.reserve(size_t(n_read_bases) + 1); S.read_mqidx.resize(n_reads + 1); S.read_start.resize(n_reads + 1);
    S.read_flags.resize(n_reads + 1); S.hap_var.resize(2 * n_var + 1); S.hap_var_flank.resize(3 * n_var + 1);
    if (with_mates) { S.read_mate_pos.resize(n_reads + 1); S.read_mate_len.resize(n_reads + 1); }
    if (pack_ref_pos) { S.hap_ref_pos.resize(size_t(n_hap_bases) + 1); S.hap_aligned.resize(n_haps + 1); }
    if (B.has_pairs) {                                   // the prior tables in window order (H * H per window, dd_pair_sum_offsets), the indel counts
        S.pair_prior.clear(); S.hap_n_indels.resize(n_haps + 1);
        for (int w = 0; w < W; w++) {
            const WindowJob &J = jobs[w];
            const size_t H = J.haps->size();
            if (!J.pairPrior || J.pairPrior->size() != H * H) throw std::string("setDeviceRealignDiploid: a job without its H x H pair prior table");
            S.pair_prior.insert(S.pair_prior.end(), J.pairPrior->begin(), J.pairPrior->end());
            for (size_t h = 0; h < H; h++) S.hap_n_indels[size_t(B.win_hap_off[w]) + h] = int32_t((*J.haps)[h].countIndels());
        }
        S.pair_prior.push_back(0.0);
    }

    const std::chrono::steady_clock::time_point t_pass1 = std::chrono::steady_clock::now();
    // ---- pass 2: the bytes, windows in parallel ----
    ValueTable qtab, mqtab;
    std::atomic<int> overflow(0);
    const unsigned nthr = pick_threads(hostThreads_, W);
    {
        auto pack_window = [&](int w, ValueCache &qc, ValueCache &mc) {
            const WindowJob &J = jobs[w];
            S.win_hap_start[size_t(w)] = J.leftPos;
            for (size_t h = 0; h < J.haps->size(); h++) {
                const Haplotype &H = (*J.haps)[h];
                const int g = B.win_hap_off[w] + int(h);
                memcpy(S.hap_seq.data() + S.hap_seq_off[size_t(g)], H.seq.data(), H.seq.size());
                if (pack_ref_pos) {                       // `hapRefPos.size() != hapSize` is getCIGAR's "Haplotype has not been aligned!"
                    const bool aligned = H.refHpos.size() == H.seq.size();
                    S.hap_aligned[size_t(g)] = aligned ? 1 : 0;
                    int32_t *hr = S.hap_ref_pos.data() + S.hap_seq_off[size_t(g)];
                    for (size_t b = 0; b < H.seq.size(); b++) hr[b] = aligned ? int32_t(H.refHpos[b]) : 0;
                }
                int32_t *hv = S.hap_var.data() + 2 * size_t(B.hap_var_off[g]);
                int32_t *hf = S.hap_var_flank.data() + 3 * size_t(B.hap_var_off[g]);
                for (std::map<int, AlignedVariant>::const_iterator it = H.indels.begin(); it != H.indels.end(); ++it) {
                    *hv++ = it->second.getStartRead(); *hv++ = it->second.getEndRead();
                    *hf++ = it->second.getLeftFlankRead(); *hf++ = it->second.getRightFlankRead();
                    *hf++ = it->second.getType() == AlignedVariant::DEL ? 1 : it->second.getType() == AlignedVariant::INS ? 2 : 0;
                }
                for (std::map<int, AlignedVariant>::const_iterator it = H.snps.begin(); it != H.snps.end(); ++it) {
                    *hv++ = it->second.getStartRead(); *hv++ = it->second.getEndRead();
                    *hf++ = 0; *hf++ = 0; *hf++ = 0;
                }
            }
            for (size_t r = 0; r < J.reads->size(); r++) {
                const Read &R = (*J.reads)[r];
                const size_t q = size_t(B.win_read_off[w]) + r;
                const size_t so = size_t(B.read_seq_off[q]);
                memcpy(S.read_seq.p + so, R.seq.seq.data(), R.size());
                uint8_t *qi = S.read_qidx.p + so;
                double lastq = -1.0;
                int lastidx = 0;
                for (size_t b = 0; b < R.qual.size(); b++) {
                    if (R.qual[b] != lastq) {                 // runs of equal qualities skip the lookup
                        const int idx = qc.get(R.qual[b], qtab);
                        if (idx < 0) { overflow.store(1); return; }
                        lastq = R.qual[b]; lastidx = idx;
                    }
                    qi[b] = uint8_t(lastidx);
                }
                const int mi = mc.get(R.mapQual, mqtab);
                if (mi < 0) { overflow.store(2); return; }
                S.read_mqidx[q] = uint8_t(mi);
                S.read_start[q] = uint32_t(R.posStat.first);      // uint32_t(read.posStat.first), ObservationModelFB.cpp:52
                S.read_flags[q] = uint8_t((R.isUnmapped() ? DD_READ_UNMAPPED : 0) | (R.isPaired() ? DD_READ_PAIRED : 0) |
                                          (R.mateIsUnmapped() ? DD_READ_MATE_UNMAPPED : 0) | (R.mateIsReverse() ? DD_READ_MATE_REVERSE : 0) |
                                          (R.mateSameTid ? DD_READ_MATE_SAME_TID : 0));
                if (with_mates) {
                    S.read_mate_pos[q] = R.matePos;
                    S.read_mate_len[q] = R.isPaired() ? R.mateLen : -1;
                }
            }
        };
        if (nthr <= 1 || W < 8) {
            ValueCache qc, mc;
            for (int w = 0; w < W; w++) pack_window(w, qc, mc);
        } else {
            std::atomic<int> next(0);
            std::vector<std::thread> pool;
            for (unsigned t = 0; t < nthr; t++)
                pool.push_back(std::thread([&]() {
                    ValueCache qc, mc;
                    for (int w0 = next.fetch_add(8); w0 < W; w0 = next.fetch_add(8))
                        for (int w = w0; w < W && w < w0 + 8; w++) pack_window(w, qc, mc);
                }));
            for (size_t t = 0; t < pool.size(); t++) pool[t].join();
        }
        if (overflow.load() == 1) throw std::string("more than 256 distinct base qualities in one batch");
        if (overflow.load() == 2) throw std::string("more than 256 distinct mapping qualities in one batch");
    }
    dd_batch Bt;
    memset(&Bt, 0, sizeof(Bt));
    Bt.n_windows = W;
    Bt.win_hap_off = B.win_hap_off.data(); Bt.win_read_off = B.win_read_off.data(); Bt.win_hap_start = S.win_hap_start.data();
    Bt.hap_seq_off = S.hap_seq_off.data(); Bt.hap_seq = S.hap_seq.data(); Bt.hap_var_off = B.hap_var_off.data();
    Bt.hap_var = n_var ? S.hap_var.data() : NULL;
    Bt.hap_var_flank = n_var ? S.hap_var_flank.data() : NULL;
    Bt.read_seq_off = B.read_seq_off.data(); Bt.read_seq = S.read_seq.p; Bt.read_qidx = S.read_qidx.p;
    Bt.read_mqidx = S.read_mqidx.data(); Bt.read_start = S.read_start.data(); Bt.read_flags = S.read_flags.data();
    double one_q = 0.5;
    Bt.n_qual = int(qtab.tab.size()); Bt.qual_table = qtab.tab.empty() ? &one_q : qtab.tab.data();
    Bt.n_mapq = int(mqtab.tab.size()); Bt.mapq_table = mqtab.tab.empty() ? &one_q : mqtab.tab.data();
    if (with_mates) {
        if (lib_p95.empty()) { lib_prob.push_back(1.0); lib_off.push_back(1); lib_p95.push_back(1.0); }   // no paired read: placeholder table
        Bt.read_mate_pos = S.read_mate_pos.data(); Bt.read_mate_len = S.read_mate_len.data(); Bt.read_lib = S.read_lib.data();
        Bt.n_libs = int(lib_p95.size()); Bt.lib_off = lib_off.data(); Bt.lib_prob = lib_prob.data(); Bt.lib_p95 = lib_p95.data();
    }

    dd_sizes sz;
    if (dd_batch_sizes(&Bt, &sz) != DD_SUCCESS) throw std::string(dd_last_error());
    B.pair_off.resize(size_t(W) + 1); B.hpos_off.resize(size_t(W) + 1); B.vc_off.resize(size_t(W) + 1);
    dd_batch_offsets(&Bt, B.pair_off.data(), B.hpos_off.data(), B.vc_off.data());

    const size_t np = size_t(sz.n_pairs) + 1;
    dd_result Rz;
    memset(&Rz, 0, sizeof(Rz));
    Rz.ll = B.ll.reserve(np); Rz.llOn = B.llOn.reserve(np); Rz.llOff = B.llOff.reserve(np); Rz.mLogBQ = B.mLogBQ.reserve(np);
    Rz.offHap = B.offHap.reserve(np); Rz.offHapHMQ = B.offHapHMQ.reserve(np); Rz.status = B.status.reserve(np);
    Rz.numIndels = B.numIndels.reserve(np); Rz.numMismatch = B.numMismatch.reserve(np); Rz.nBQT = B.nBQT.reserve(np);
    Rz.nmmBQT = B.nmmBQT.reserve(np); Rz.nMMLeft = B.nMMLeft.reserve(np); Rz.nMMRight = B.nMMRight.reserve(np);
    Rz.firstBase = B.firstBase.reserve(np); Rz.lastBase = B.lastBase.reserve(np);
    Rz.onHap = NULL;                                    // derived from offHapHMQ on the host (WindowLikelihoods::onHap)
    Rz.var_fcov = B.fcov.reserve(size_t(sz.var_cov_len) + 1); Rz.var_covered = B.vcov.reserve(size_t(sz.var_cov_len) + 1);
    if (B.has_hpos) Rz.hpos = B.hpos.reserve(size_t(sz.hpos_len) + 1);
    dd_cigar_result Cg;
    memset(&Cg, 0, sizeof(Cg));
    if (B.has_cigars) {
        Cg.n_ops = B.cig_n_ops.reserve(np); Cg.ref_off = B.cig_ref_off.reserve(np); Cg.status = B.cig_status.reserve(np);
        Cg.ops = B.cig_ops.reserve(np * size_t(B.cig_cap));
    }
    dd_realign_result Rl;
    memset(&Rl, 0, sizeof(Rl));
    if (B.has_realign) {
        const size_t nr = n_reads + 1;
        Rl.hap = B.rl_hap.reserve(nr); Rl.status = B.rl_status.reserve(nr); Rl.n_ops = B.rl_n_ops.reserve(nr); Rl.ref_off = B.rl_ref_off.reserve(nr);
        Rl.ops = B.rl_ops.reserve(nr * size_t(B.cig_cap));
        if (!B.has_pairs) Rz.onHap = B.on_hap.reserve(nr);   // the pooled rule reads it on the device
    }
    dd_diploid_pair_result Dp;
    memset(&Dp, 0, sizeof(Dp));
    if (B.has_pairs) {
        const size_t nw = size_t(W) + 1;
        Dp.pair = B.dp_pair.reserve(2 * nw); Dp.state = B.dp_state.reserve(nw); Dp.best = B.dp_best.reserve(nw); Dp.gap = B.dp_gap.reserve(nw);
        Dp.margin = B.dp_margin.reserve(nw);
    }
    lastRealignBytes = (B.has_realign ? n_reads * (16 + 4 * size_t(B.cig_cap)) : 0) + (B.has_pairs ? size_t(W) * 36 : 0);
    lastHposBytes = B.has_hpos ? size_t(sz.hpos_len) * sizeof(int16_t) : 0;
    lastCigarBytes = B.has_cigars ? size_t(sz.n_pairs) * (12 + 4 * size_t(B.cig_cap)) : 0;
    lastIndelKeyBytes = B.has_keys ? size_t(sz.n_pairs) * sizeof(int16_t) : 0;
    auditReport_ = AuditReport();
    dd_params P = to_abi(params);
    if (faster) P.mapUnmappedReads = 0;                 // ObservationModelS has no insert-size prior
    // the entries' option bits (the audits take the long-window bit alone; the wide bit goes along only where it is needed)
    const uint32_t wideOpt = wideDeletions_ && P.maxLengthDel > DD_MAX_LENGTH_DEL ? DD_OPT_WIDE_DELETIONS : 0u;
    const uint32_t mainOpt = (longWindows_ ? DD_OPT_LONG_WINDOWS : 0u) | wideOpt, fasterOpt = (longWindowsFaster_ ? DD_OPT_LONG_WINDOWS_FASTER : 0u) | wideOpt;
    const std::chrono::steady_clock::time_point t_packed = std::chrono::steady_clock::now();
    if (getenv("DD_TIMING"))
        fprintf(stderr, "pack_timing: windows=%d pass1=%.2fms pass2+alloc=%.2fms\n", W, std::chrono::duration<double, std::milli>(t_pass1 - t_start).count(),
                std::chrono::duration<double, std::milli>(t_packed - t_pass1).count());
    if (B.has_pairs) {                                   // (also without pairs: the windows' states and the reads' marks are still due)
        typedef int (*Entry)(const dd_params *, const dd_batch *, dd_result *, const double *, const int32_t *, const int32_t *, const uint8_t *,
                             const dd_diploid_pair_result *, const dd_realign_result *, int, int, uint32_t);
        const int rc = reinterpret_cast<Entry>(diploidEntry_)(&P, &Bt, &Rz, S.pair_prior.data(), S.hap_n_indels.data(), S.hap_ref_pos.data(),
                                                              S.hap_aligned.data(), &Dp, &Rl, B.cig_cap, device_, mainOpt);
        if (rc != DD_SUCCESS) throw std::string("dd_compute_likelihoods_realign_diploid: ") + dd_last_error();
    } else if (B.has_realign) {                          // (also without pairs: reads of windows without haplotypes are marked)
        const int rc = dd_compute_likelihoods_realign(&P, &Bt, &Rz, DD_REALIGN_FIRST_MAX, NULL, NULL, S.hap_ref_pos.data(), S.hap_aligned.data(), &Rl,
                                                      B.cig_cap, device_, mainOpt);
        if (rc != DD_SUCCESS) throw std::string("dd_compute_likelihoods_realign: ") + dd_last_error();
    } else if (sz.n_pairs > 0 && B.has_cigars) {
        const int rc = dd_compute_likelihoods_cigars(&P, &Bt, &Rz, S.hap_ref_pos.data(), S.hap_aligned.data(), &Cg, B.cig_cap, device_, mainOpt);
        if (rc != DD_SUCCESS) throw std::string("dd_compute_likelihoods_cigars: ") + dd_last_error();
    } else if (sz.n_pairs > 0 && faster && auditFaster_ > 0 && auditFasterCall_) {
        const int rc = auditFasterCall_(*this, &P, &Bt, &Rz, B.has_keys ? B.indel_keys.reserve(np) : NULL, longWindowsFaster_ ? DD_OPT_LONG_WINDOWS_FASTER : 0u);
        if (rc != DD_SUCCESS) throw std::string("dd_compute_likelihoods_faster_audit: ") + dd_last_error();
    } else if (sz.n_pairs > 0 && B.has_keys) {
        typedef int (*Entry)(const dd_params *, const dd_batch *, dd_result *, int16_t *, int, uint32_t);
        const int rc = reinterpret_cast<Entry>(indelKeysEntry_)(&P, &Bt, &Rz, B.indel_keys.reserve(np), device_, fasterOpt);
        if (rc != DD_SUCCESS) throw std::string("dd_compute_likelihoods_faster_keys: ") + dd_last_error();
    } else if (sz.n_pairs > 0 && !faster && audit_ > 0 && auditCall_) {
        const int rc = auditCall_(*this, &P, &Bt, &Rz, longWindows_ ? DD_OPT_LONG_WINDOWS : 0u);
        if (rc != DD_SUCCESS) throw std::string("dd_compute_likelihoods_audit: ") + dd_last_error();
    } else if (sz.n_pairs > 0) {
        const int rc = faster ? (fasterOpt ? dd_compute_likelihoods_faster_ex(&P, &Bt, &Rz, device_, fasterOpt) : dd_compute_likelihoods_faster(&P, &Bt, &Rz, device_))
                     : mainOpt ? dd_compute_likelihoods_ex(&P, &Bt, &Rz, device_, mainOpt) : dd_compute_likelihoods(&P, &Bt, &Rz, device_);
        if (rc != DD_SUCCESS) throw std::string(faster ? (fasterOpt ? "dd_compute_likelihoods_faster_ex: " : "dd_compute_likelihoods_faster: ") : mainOpt ? "dd_compute_likelihoods_ex: " : "dd_compute_likelihoods: ") + dd_last_error();
    }

    const std::chrono::steady_clock::time_point t_device = std::chrono::steady_clock::now();
    // ---- per window: the error the reference's loop would have stopped at (first pair in liks[h][r] order that is not OK),
    // the lazy view, and — for jobs that bring the reference's containers — every record ----
    const std::shared_ptr<const BatchBlock> cblk = blk;
    auto finish_window = [&](int w) {
        WindowJob &J = jobs[w];
        const size_t H = J.haps->size(), Rn = J.reads->size();
        const bool eager = J.liks != NULL;
        if (J.onHap) *J.onHap = std::vector<int>(Rn, 0);                                                        // DInDel.cpp:1710
        if (eager) *J.liks = std::vector<std::vector<MLAlignment> >(H, std::vector<MLAlignment>(Rn));           // DInDel.cpp:1714
        for (size_t h = 0; h < H && J.error.empty(); h++) {
            for (size_t r = 0; r < Rn; r++) {
                const int64_t p = B.pair_off[w] + int64_t(h) * int64_t(Rn) + int64_t(r);
                const int st = B.status[size_t(p)];
                if (st == DD_PAIR_HAPSIZE) { J.error = "hapSize error."; break; }   // ObservationModelFB.cpp:47, Faster.cpp:47
                if (st == DD_PAIR_UNSUPPORTED) {      // this window only; the caller skips it like a window that threw (DInDel.cpp:1369-1374)
                    J.error = (longWindows_ && !faster)
                                  ? "window outside the GPU kernel limits (haplotype > 4094 bp, read > 4096 bp, an empty sequence or a haplotype byte without a symbol id)"
                                  : "window outside the GPU kernel limits (haplotype > 766 bp, read > 1024 bp or an empty sequence)";
                    break;
                }
                if (faster && st != DD_PAIR_OK) { J.error = "HapHash string too short"; break; }   // Haplotype.hpp:341
                if (eager) fill_record(B, w, h, r, (*J.haps)[h], (*J.reads)[r], (*J.liks)[h][r]);
                if (J.onHap && !B.offHapHMQ[size_t(p)]) (*J.onHap)[r] = 1;                // DInDel.cpp:1720
                if (faster) continue;                                                     // computeLikelihoodsFaster has no ll checks
                if (st == DD_PAIR_LLPOS) {                                                // DInDel.cpp:1722-1731
                    if (throwOnPositive_) { J.error = "Likelihood>0"; break; }
                    std::cout << "hidx: " << h << " r: " << r << std::endl;
                    std::cerr << "Likelihood>0" << std::endl;
                    exit(1);
                }
                if (st == DD_PAIR_NAN) {                                                  // DInDel.cpp:1732-1735
                    std::cout << "NAN/Inf error" << std::endl;
                    J.error = "Nan detected";
                    break;
                }
            }
        }
        if (J.error.empty()) {
            J.result.blk_ = cblk; J.result.w_ = w; J.result.haps_ = J.haps; J.result.reads_ = J.reads;
            J.result.leftPos_ = J.leftPos; J.result.eng_ = this;
        }
    };
    parallel_windows(W, pick_threads(hostThreads_, W), 4, finish_window);
    const std::chrono::steady_clock::time_point t_end = std::chrono::steady_clock::now();
    lastPackSeconds = std::chrono::duration<double>(t_packed - t_start).count();
    lastDeviceSeconds = std::chrono::duration<double>(t_device - t_packed).count();
    lastUnpackSeconds = std::chrono::duration<double>(t_end - t_device).count();
}

} // namespace dindel
