// compute_likelihoods.hpp — C++ host adapter with the reference's operator interface for the hot path.
//
//   void DetInDel::computeLikelihoods(const vector<Haplotype>&, const vector<Read>&,
//                                     vector<vector<MLAlignment> >& liks, uint32_t leftPos, uint32_t rightPos,
//                                     vector<int>& onHap);                 reference DInDel.hpp:136, DInDel.cpp:1707-1739
//
// Same argument meaning, same outputs (liks[hidx][r], onHap[r]) and the same error behaviour:
//   * haplotype shorter than maxLengthDel  -> throws std::string("hapSize error.")   (ObservationModelFB.cpp:47)
//   * NaN / Inf log-likelihood             -> throws std::string("Nan detected")     (DInDel.cpp:1732-1735)
//   * log-likelihood > 0.1                 -> "Likelihood>0" on stderr, exit(1)      (DInDel.cpp:1722-1731)
//                                             (setThrowOnPositiveLikelihood(true) turns the exit into a throw)
//   * window shape outside the kernel limits (haplotype > 766 bp, read > 1024 bp, empty sequence — with setLongWindows(true) in the main
//     model: haplotype > 4,094 bp, read > 4,096 bp, empty sequence, a haplotype byte without a symbol id; no reference counterpart)
//     -> throws std::string("window outside the GPU kernel limits ...") for THAT window only
// All arithmetic runs on the GPU through the C ABI (include/dindel_hmm.h); this class only packs the
// windows, calls dd_compute_likelihoods and hands the records back.
//
// Two ways to receive a batch's records:
//   * eager  — WindowJob::liks / onHap point at the reference's containers: every MLAlignment (five std::map's, two
//              strings, a vector) is rebuilt.  The literal drop-in; the host spends ~0.1 us per read base on it.
//   * lazy   — WindowJob::liks == NULL: the job's WindowLikelihoods view exposes every scalar of every record straight from
//              the batch's result block (what the reductions of DInDel.cpp:2933-3660 read: ll, offHap, numIndels, the QC
//              counters, the covered flags) and builds a full MLAlignment only for the pairs a consumer asks for (get()).
#ifndef DINDEL_COMPUTE_LIKELIHOODS_HPP
#define DINDEL_COMPUTE_LIKELIHOODS_HPP
#include <cstdint>
#include <memory>
#include <utility>
#include <vector>
#include "dindel_types.hpp"

namespace dindel {

class LikelihoodEngine;
struct BatchBlock;                       // flat result arrays of one batch call (compute_likelihoods.cpp)
struct PackScratch;                      // flat input arrays of one batch call

// Read-only view of one window's records inside a batch's result block.  Cheap to copy; keeps the block alive.
class WindowLikelihoods {
public:
    WindowLikelihoods() : w_(-1), haps_(NULL), reads_(NULL), leftPos_(0), eng_(NULL) {}
    bool valid() const { return w_ >= 0 && bool(blk_); }
    size_t numHaps() const;
    size_t numReads() const;
    // the scalars of liks[h][r] (MLAlignment.hpp:35-75)
    double ll(size_t h, size_t r) const;
    double llOn(size_t h, size_t r) const;
    double llOff(size_t h, size_t r) const;
    double mLogBQ(size_t h, size_t r) const;
    bool offHap(size_t h, size_t r) const;
    bool offHapHMQ(size_t h, size_t r) const;
    int numIndels(size_t h, size_t r) const;      // == liks[h][r].indels.size() for the main model (one key per event)
    int indelCount(size_t h, size_t r) const;     // liks[h][r].indels.size() for either model (the --faster model leaves numIndels 0
                                                  // and may key several events at one position): what DInDel.cpp:3529 reads.  With
                                                  // device indel keys it is the device's value; for a pair with more than 64 keys
                                                  // the window is recomputed with alignments, by an engine of the call's own, and
                                                  // counted (indelKeyFallbacks())
    // Device indel keys (LikelihoodEngine::setDeviceIndelKeys): the --faster batch brought one int16 per pair back instead of the alignments
    bool hasDeviceIndelKeys() const;
    int deviceIndelKeys(size_t h, size_t r) const;   // the raw value: the count, DD_INDEL_KEYS_OVERFLOW or DD_INDEL_KEYS_NOT_COMPUTED
    int numMismatch(size_t h, size_t r) const;
    int nBQT(size_t h, size_t r) const;
    int nmmBQT(size_t h, size_t r) const;
    int nMMLeft(size_t h, size_t r) const;
    int nMMRight(size_t h, size_t r) const;
    int firstBase(size_t h, size_t r) const;
    int lastBase(size_t h, size_t r) const;
    int onHap(size_t r) const;                    // DInDel.cpp:1720
    // liks[h][r].hapIndelCovered[key] / hapSNPCovered[key] (false when the haplotype has no such variant, like the
    // reference's find()-then-test at DInDel.cpp:3158, :3539) and the filterHaplotypes coverage flag of a haplotype indel
    bool hapIndelCovered(size_t h, size_t r, int key) const;
    bool hapSNPCovered(size_t h, size_t r, int key) const;
    bool hapIndelFilterCovered(size_t h, size_t r, int key) const;
    // the same flags by slot, for loops over the reads of one (haplotype, variant): slot = varSlot(h, key, snp) once,
    // then coveredAt / filterCoveredAt per read (slot < 0: false)
    int varSlot(size_t h, int key, bool snp) const;
    bool coveredAt(size_t h, size_t r, int slot) const;
    bool filterCoveredAt(size_t h, size_t r, int slot) const;
    // One haplotype's scalars as plain rows indexed by read (x[r] == x(h, r)), and its covered flags: flag of variant slot s for read r
    // is vcov[r * nv + s] (fcov likewise).  For loops over the reads; valid as long as the view is.
    struct Rows {
        const double *ll, *llOn, *llOff, *mLogBQ;
        const uint8_t *offHap, *offHapHMQ, *vcov, *fcov;
        const int16_t *numIndels, *numMismatch, *nBQT, *nmmBQT, *nMMLeft, *nMMRight, *firstBase, *lastBase;
        int nv;
        bool covered(size_t r, int slot) const { return slot >= 0 && vcov[r * size_t(nv) + size_t(slot)] != 0; }
        bool filterCovered(size_t r, int slot) const { return slot >= 0 && fcov[r * size_t(nv) + size_t(slot)] != 0; }
    };
    Rows rows(size_t h) const;
    // the full record of one pair, built on demand (variant maps, align string, hpos).  If the batch was run without
    // alignments (setKeepAlignments(false)) the window is recomputed once through the engine and cached.
    MLAlignment get(size_t h, size_t r) const;
    // Device CIGARs (LikelihoodEngine::setDeviceCigars): getCIGAR of pair (h, r) as the device computed it from the alignment it kept —
    // status (DD_CIGAR_* of include/dindel_hmm.h: 0, the code of the string getCIGAR throws, DD_CIGAR_OVERFLOW, DD_CIGAR_NOT_COMPUTED),
    // the operation count (also beyond cigarOpsCap()), the first min(count, cap) BAM words (len << 4 | op) and the reference offset of the
    // first aligned base (-1: none).  Straight from the batch's result block, like the scalars.
    bool hasDeviceCigars() const;
    int cigarOpsCap() const;
    int cigarStatus(size_t h, size_t r) const;
    int cigarNumOps(size_t h, size_t r) const;
    const uint32_t *cigarOps(size_t h, size_t r) const;
    int cigarRefOff(size_t h, size_t r) const;
    // Device realign (LikelihoodEngine::setDeviceRealign): per READ the haplotype the device chose for it by the pooled rule
    // (DD_REALIGN_FIRST_MAX; -1: none) and that pair's CIGAR: status (DD_CIGAR_* of the chosen pair, or DD_REALIGN_OFF_HAP /
    // DD_REALIGN_NO_HAPS), operation count, the first min(count, cigarOpsCap()) BAM words and the reference offset.
    bool hasDeviceRealign() const;
    int realignHap(size_t r) const;
    int realignStatus(size_t r) const;
    int realignNumOps(size_t r) const;
    const uint32_t *realignOps(size_t r) const;
    int realignRefOff(size_t r) const;
    // Device pair (LikelihoodEngine::setDeviceRealignDiploid): the window's MAP haplotype pair as the device chose and certified it
    // (dd_diploid_pairs_device): pairState() is a DD_DIPPAIR_* of include/dindel_hmm.h, devicePair() the pair when the state is
    // DD_DIPPAIR_CERTIFIED and (-1, -1) otherwise.  The realign rows above are then the diploid rule's (DD_REALIGN_PAIR) for that pair; the
    // reads of a window that is not certified carry DD_REALIGN_BAD_PAIR.
    bool hasDevicePair() const;
    int pairState() const;
    std::pair<int, int> devicePair() const;
    // A one-window view over hand-made realign rows (and, with hpos, hand-made per-base alignments for get(): one entry per (haplotype,
    // read base), haplotype-major).  For tests of the consumers of these views; `haps` and `reads` must outlive it.
    static WindowLikelihoods handMadeRealign(const std::vector<Haplotype> &haps, const std::vector<Read> &reads, int opsCap, const int32_t *hap,
                                             const int32_t *status, const int32_t *nOps, const uint32_t *ops, const int32_t *refOff,
                                             const int16_t *hpos, const double *ll = NULL, int pairState = -1, const int32_t *pair = NULL);
    // ... ll (may be NULL: all 0): the pairs' likelihoods, haplotype-major; pairState >= 0: the view also carries a device pair.
    // A one-window view of the --faster model over hand-made per-base alignments (hpos: haplotype-major, or NULL: none came back) and
    // hand-made device indel keys (keys: one per pair, haplotype-major, or NULL).  eng: the engine get() recomputes the window with when
    // the view has no alignments, and whose parameters and device indelCount's own recomputation takes (may be NULL: defaults, device 0).  For tests of indelCount; `haps` and `reads` must outlive it.
    static WindowLikelihoods handMadeFaster(const std::vector<Haplotype> &haps, const std::vector<Read> &reads, const int16_t *hpos,
                                            const int16_t *keys, LikelihoodEngine *eng = NULL);
    // all records, as the eager path fills them
    void toLiks(std::vector<std::vector<MLAlignment> > &liks, std::vector<int> &onHap) const;

private:
    friend class LikelihoodEngine;
    int64_t pair(size_t h, size_t r) const;
    std::shared_ptr<const BatchBlock> blk_;
    mutable std::shared_ptr<const BatchBlock> full_;   // recomputed one-window block (no-alignment batches)
    int w_;
    const std::vector<Haplotype> *haps_;
    const std::vector<Read> *reads_;
    uint32_t leftPos_;
    LikelihoodEngine *eng_;
};

struct WindowJob {                      // one call of the reference's computeLikelihoods
    WindowJob() : haps(NULL), reads(NULL), leftPos(0), rightPos(0), liks(NULL), onHap(NULL), pairPrior(NULL) {}
    const std::vector<Haplotype> *haps;
    const std::vector<Read> *reads;
    uint32_t leftPos, rightPos;
    std::vector<std::vector<MLAlignment> > *liks;   // OUT (eager); NULL = lazy: use `result`
    std::vector<int> *onHap;                        // OUT (eager); may be NULL
    const std::vector<double> *pairPrior;           // setDeviceRealignDiploid: getHaplotypePrior(h1, h2) at [h1 * haps->size() + h2], h1 <= h2
    WindowLikelihoods result;                       // OUT: always set (unless the window has an error)
    std::string error;                              // OUT: empty, or the string the reference would have thrown
};

class LikelihoodEngine {
public:
    explicit LikelihoodEngine(const ObservationModelParameters &obsParams, int device = 0)
        : params(obsParams), device_(device), throwOnPositive_(false), hostThreads_(0), keepAlignments_(true) {}

    ObservationModelParameters params;   // the reference passes this->params.obsParams implicitly (DInDel.cpp:1718)

    // drop-in for one window
    void computeLikelihoods(const std::vector<Haplotype> &haps, const std::vector<Read> &reads,
                            std::vector<std::vector<MLAlignment> > &liks, uint32_t leftPos, uint32_t rightPos,
                            std::vector<int> &onHap);

    // the batched form a GPU wants: prepare-N -> one launch -> reduce-N in order.  A window that would have
    // thrown gets its message in WindowJob::error (the caller turns it into the "skipped" row, DInDel.cpp:1361-1408).
    void computeLikelihoodsBatch(std::vector<WindowJob> &jobs);

    // DetInDel::computeLikelihoodsFaster (reference DInDel.cpp:1790-1833): the --faster model, ObservationModelS.
    // Throws std::string("hapSize error.") (Faster.cpp:47) or std::string("HapHash string too short")
    // (Haplotype.hpp:341, read shorter than the 4-mer); no likelihood checks, as in the reference.
    void computeLikelihoodsFaster(const std::vector<Haplotype> &haps, const std::vector<Read> &reads,
                                  std::vector<std::vector<MLAlignment> > &liks, uint32_t leftPos, uint32_t rightPos,
                                  std::vector<int> &onHap);
    void computeLikelihoodsFasterBatch(std::vector<WindowJob> &jobs);

    void setThrowOnPositiveLikelihood(bool v) { throwOnPositive_ = v; }
    // host threads packing the windows / rebuilding eager records (0 = min(16, hardware threads))
    void setHostThreads(int n) { hostThreads_ = n; }
    // false: the per-base alignments (hpos, 45 % of the result bytes) stay on the device side of the call; lazy views
    // recompute a window on the first get().  Scalars, covered flags and onHap are always delivered.
    void setKeepAlignments(bool v) { keepAlignments_ = v; }
    // true: windows beyond the main kernels' limits (haplotypes up to 4,094 bp, reads up to 4,096 bp; with maxLengthIndel >= 12 haplotypes
    // over 574 bp) are computed by the long-window kernel (dd_compute_likelihoods_ex, DD_OPT_LONG_WINDOWS) instead of being reported as
    // windows that threw.  Main model only; default off.
    void setLongWindows(bool v) { longWindows_ = v; }
    bool longWindows() const { return longWindows_; }
    // true: the same for the --faster model, which setLongWindows does not touch: windows with a haplotype of 767..4,094 bp or a read of
    // 1,025..4,096 bp are computed by that model's long-window kernel (dd_compute_likelihoods_faster_ex, DD_OPT_LONG_WINDOWS_FASTER).
    // No effect on the main model; default off.
    void setLongWindowsFaster(bool v) { longWindowsFaster_ = v; }
    bool longWindowsFaster() const { return longWindowsFaster_; }
    // true: maxLengthDel above 31 is accepted (DD_OPT_WIDE_DELETIONS).  Main model: with setLongWindows(true) (the library refuses the
    // option without it) every window within the long limits is then computed by the long-window kernel's wide build.  --faster model: the
    // value is only compared with the haplotype length, the kernels run unchanged.  With maxLengthDel <= 31 it changes nothing; audits
    // (setAudit, setAuditFaster) are not given the option and keep refusing such a value.  Default off.
    void setWideDeletions(bool v) { wideDeletions_ = v; }
    bool wideDeletions() const { return wideDeletions_; }
    // true: computeLikelihoodsBatch packs every haplotype's refHpos and asks for the pairs' CIGARs (dd_compute_likelihoods_cigars) INSTEAD of
    // their per-base alignments: 4 opsCap + 12 bytes per pair come back instead of 2 L, and the lazy views expose them (hasDeviceCigars()).
    // get() on such a view recomputes the window with alignments, as for setKeepAlignments(false).  Main model, lazy jobs only: a batch with an
    // eager job, and the --faster model, run as without it.  Default off.
    void setDeviceCigars(bool v, int opsCap = 8) { deviceCigars_ = v; cigarOpsCap_ = opsCap < 1 ? 1 : opsCap; }
    bool deviceCigars() const { return deviceCigars_; }
    // true: computeLikelihoodsBatch asks for the realigned reads instead (dd_compute_likelihoods_realign, DD_REALIGN_FIRST_MAX): the device
    // picks each read's haplotype by the pooled rule and only that pair's CIGAR comes back, 4 opsCap + 16 bytes per READ; the lazy views
    // expose them (hasDeviceRealign()) and carry neither alignments nor per-pair CIGARs.  Wins over setDeviceCigars.  Main model, lazy jobs
    // only: a batch with an eager job, and the --faster model, run as without it.  Default off.
    void setDeviceRealign(bool v, int opsCap = 8) { deviceRealign_ = v; if (v) cigarOpsCap_ = opsCap < 1 ? 1 : opsCap; }
    bool deviceRealign() const { return deviceRealign_; }
    // true: computeLikelihoodsBatch asks for the diploid step's realigned reads (dd_compute_likelihoods_realign_diploid): the device picks and
    // certifies every window's MAP haplotype pair from WindowJob::pairPrior (required on every job), then each read's haplotype by the diploid
    // rule; the views expose pairState(), devicePair() and the rows of hasDeviceRealign().  Wins over setDeviceRealign and setDeviceCigars.
    // Main model, lazy jobs only, like them.  Default off.
    // (Defined in device_pair.cpp, which binds the C ABI's entry: a program that stubs the C ABI without that entry and never sets this links.)
    void setDeviceRealignDiploid(bool v, int opsCap = 8);
    bool deviceRealignDiploid() const { return deviceRealignDiploid_; }
    // true: computeLikelihoodsFasterBatch asks for the pairs' indel-map key counts (dd_compute_likelihoods_faster_keys) INSTEAD of their
    // per-base alignments: 2 bytes per pair come back instead of 2 L, and WindowLikelihoods::indelCount returns the device's value.  get() on
    // such a view recomputes the window with alignments, as for setKeepAlignments(false); indelCount does the same, with an engine of its
    // own (it is called from reduce threads), and only for a pair with more than 64 distinct keys.  --faster model, lazy jobs only: a batch with an eager job, and the main model, run as without it.  Default off.
    // (Defined in device_indel_keys.cpp, which binds the C ABI's entry, like setDeviceRealignDiploid.)
    void setDeviceIndelKeys(bool v);
    bool deviceIndelKeys() const { return deviceIndelKeys_; }
    // pairs whose indelCount was recomputed with alignments because the device reported more than 64 keys (process-wide, all engines)
    static long indelKeyFallbacks();
    // Audit (main model): every computeLikelihoodsBatch call that goes through the plain likelihood entry has windowsPerCall of its windows
    // (0 = off) recomputed by the long-window kernel and compared with the main kernels' results on the device
    // (dd_compute_likelihoods_audit; the sample is a function of `seed` and the batch).  The results of the call are what they are without
    // it; auditReport() is the last such call's report.  Calls that ask for device CIGARs, realigned reads or the diploid pair take no
    // audit: their report is empty (the --faster model has setAuditFaster, below).  Default off.
    // (Defined in device_audit.cpp, which binds the C ABI's entries, like setDeviceIndelKeys.)
    struct AuditDifference { int job, field; long long pair /* inside the job's window */, index; unsigned long long primaryBits, shadowBits; };
    struct AuditReport {
        long long windows = 0, pairs = 0, mismatches = 0;     // windows and pairs compared; differences found (all of them)
        std::vector<AuditDifference> differences;             // the first 64 of them
    };
    void setAudit(int windowsPerCall, unsigned long long seed);
    int audit() const { return audit_; }
    // Audit of the --faster model: every --faster call that goes through the plain or the key entry (setDeviceIndelKeys) has windowsPerCall of
    // the windows it computes (its long windows too, with setLongWindowsFaster) recomputed by the independent shadow kernel and compared on the
    // device (dd_compute_likelihoods_faster_audit).  Results, seed, auditReport() and the test hook as setAudit's.  Default off.
    void setAuditFaster(int windowsPerCall, unsigned long long seed);
    int auditFaster() const { return auditFaster_; }
    const AuditReport &auditReport() const { return auditReport_; }
    static const char *auditFieldName(int field);
    // test hook: the next audited call inverts one bit of the device copy of ll of job `job`'s first pair in front of the audit (of the
    // first audited window if that job is not in the sample) and restores it behind it: a caller's handling of a difference can be tested
    // without anything going wrong on the device
    void setAuditInject(int job) { auditInject_ = job; }
    // optional: have the calling thread's device cache (arena, staging mirror, streams) of this engine's device made now, for batches of
    // about `pairs` (haplotype, read) pairs — e.g. while the first batch is still being prepared.  Throws like the batch calls.
    void warmUp(size_t pairs);

    // wall time of the last batch call's three stages (tools/host_adapter_bench.cpp, bench.py)
    double lastPackSeconds = 0.0, lastDeviceSeconds = 0.0, lastUnpackSeconds = 0.0;
    // bytes of per-base alignments (hpos) and of CIGAR arrays the last batch call brought back from the device
    size_t lastHposBytes = 0, lastCigarBytes = 0;
    size_t lastRealignBytes = 0;         // ... and of the realigned reads' arrays (setDeviceRealign)
    size_t lastIndelKeyBytes = 0;        // ... and of the indel-map key counts (setDeviceIndelKeys)

    // ObservationModelFBMax::reportVariants (ObservationModelFB.cpp:1351-1475) from the device's hpos: fills
    // hpos, indels, snps, align, firstBase/lastBase, counters and the covered maps.  Exposed for tests.
    static void rebuildAlignment(const Haplotype &hap, const Read &read, const int16_t *hpos,
                                 const ObservationModelParameters &p, MLAlignment &ml);

    // ObservationModelS::reportVariants (Faster.cpp:579-681) from the device's hpos (inserted bases carry the key the
    // model assigned them, Faster.cpp:552-571, so overhanging bases parked on the last haplotype base do not confuse it).
    static void rebuildAlignmentFaster(const Haplotype &hap, const Read &read, const int16_t *hpos,
                                       const ObservationModelParameters &p, MLAlignment &ml);

private:
    friend class WindowLikelihoods;
    void runBatch(std::vector<WindowJob> &jobs, bool faster);
    int device_;
    bool throwOnPositive_;
    int hostThreads_;
    bool keepAlignments_;
    bool longWindows_ = false;
    bool longWindowsFaster_ = false;
    bool wideDeletions_ = false;
    bool deviceCigars_ = false;
    bool deviceRealign_ = false;
    bool deviceRealignDiploid_ = false;
    void (*diploidEntry_)() = nullptr;   // dd_compute_likelihoods_realign_diploid, once setDeviceRealignDiploid has been called
    bool deviceIndelKeys_ = false;
    void (*indelKeysEntry_)() = nullptr; // dd_compute_likelihoods_faster_keys, once setDeviceIndelKeys has been called
    int audit_ = 0, auditFaster_ = 0, auditInject_ = -1;
    unsigned long long auditSeed_ = 0;
    AuditReport auditReport_;
    static int auditedCall(LikelihoodEngine &E, const void *params, const void *batch, void *result, unsigned options);
    int (*auditCall_)(LikelihoodEngine &, const void *, const void *, void *, unsigned) = nullptr;   // auditedCall, once setAudit has been called
    static int auditedFasterCall(LikelihoodEngine &E, const void *params, const void *batch, void *result, short *keys, unsigned options);
    int (*auditFasterCall_)(LikelihoodEngine &, const void *, const void *, void *, short *, unsigned) = nullptr;   // ... setAuditFaster
    int cigarOpsCap_ = 8;
    std::vector<std::shared_ptr<BatchBlock> > spare_;   // result blocks of earlier calls; one nobody references any more is reused (warm pages)
    unsigned spareNext_ = 0;
    std::shared_ptr<PackScratch> scratch_;   // the packed inputs' buffers, reused between calls
};

} // namespace dindel
#endif
