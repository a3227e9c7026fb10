// pooled_em.hpp — DetInDel::estimateHaplotypeFrequenciesBayesEM (reference DInDel.cpp:2103-2930), the --doPooled analysis, on the records
// of one window: everything around the EM loop.  The loop itself (:2412-2543) runs in the library, one slot per set of active variants
// (dd_pooled_em on the device, dd_pooled_em_host on the CPU: csrc/pooled_math.h, the same bits either way).
//   pooledWindowOf  what the analysis reads of a window's records, taken from the batch's view (with filterHaplotypes, :2142-2150)
//   pooledPlan    allVariants, the active sets of `all` / `singlevariant` / `priorpersite`, logpriors, masks   :2142-2408
//   pooledRunEM   the slots of a batch of windows through the library, results back into the plans
//   pooledLines   logz, post, hapFreqs, per variant the marginal posterior and frequency, the marginalised pair prior, per-pool
//                 genotype likelihoods, msq, strand counts, and the window's .glf.txt lines                                       :2541-2816
// This part uses glibc and the reference's term order (DESIGN 8 point 2).  --opl files and the stdout chatter are not written.
#ifndef DINDEL_POOLED_EM_HPP
#define DINDEL_POOLED_EM_HPP
#include <functional>
#include <map>
#include <string>
#include <vector>
#include "compute_likelihoods.hpp"
#include "diploid_glf.hpp"

namespace dindel {

struct PooledParameters {                 // DetInDel::Parameters fields the analysis looks at (defaults: DInDel.hpp:200, :244, DInDel.cpp:4142)
    PooledParameters() : a0(0.001), EMtol(1e-4), bayesType("singlevariant") {}
    double a0, EMtol;
    std::string bayesType;
};

bool knownBayesType(const std::string &program);

// What the analysis reads of a window's records: plain data, so that everything below also runs without a device behind it.
struct PooledWindow {
    PooledWindow() : nh(0), nr(0) {}
    size_t nh, nr;
    std::vector<double> ll;                            // [h * nr + r]: liks[h][r].ll
    std::vector<uint8_t> offHap;                       // [h * nr + r]
    std::vector<int> filtered;                         // [nh], filterHaplotypes
    std::map<PAV, VariantCoverage> varCoverage;        // filterHaplotypes
    // liks[h][r].hapIndelCovered[pos] (snp: hapSNPCovered[pos]); false when the record has no such key
    std::function<bool(size_t h, size_t r, int pos, bool snp)> covered;
};
void pooledWindowOf(const std::vector<Haplotype> &haps, const std::vector<Read> &reads, const WindowLikelihoods &liks, const DiploidParameters &params,
                    PooledWindow &win);                // pooled_em_view.cpp

struct PooledPlan {
    PooledPlan() : nav(0), ready(false) {}
    std::vector<PAV> allVariants;                      // in std::set<PAV> order
    int nav;                                           // number of active sets
    std::vector<double> logpriors;                     // [nav]
    std::vector<int> active, hapHasVar;                // [nav * nv], [nh * nv]
    std::vector<uint8_t> compat;                       // [nav * nh]: the slots' masks
    std::vector<double> logliks, freqs;                // [nav], [nav * nh]: what the slots returned
    bool ready;                                        // the slots' results are in
};

// The sets and masks of one window.  An unknown `program` prints "Unknown EM option" and ends the process with status 1, like the reference.
void pooledPlan(const std::vector<Haplotype> &haps, const PooledWindow &win, uint32_t leftPos, const AlignedCandidates &candidateVariants,
                const DiploidParameters &params, const std::string &program, PooledPlan &plan);

// One library call for the slots of all the plans (wins[i] belongs to plans[i]): hostEM false = dd_pooled_em on `device`, true =
// dd_pooled_em_host on `threads` threads.  Throws std::runtime_error with the library's message.
void pooledRunEM(const std::vector<PooledPlan *> &plans, const std::vector<const PooledWindow *> &wins, const PooledParameters &pp,
                 bool hostEM, int device, int threads);

// The window's lines (plan.ready).  numPools: myBams.size().
void pooledLines(const std::vector<Haplotype> &haps, const std::vector<Read> &reads, const PooledWindow &win, const PooledPlan &plan,
                 uint32_t candPos, uint32_t leftPos, uint32_t rightPos, OutputData &glfData, int index, const std::string &tid,
                 const AlignedCandidates &candidateVariants, const DiploidParameters &params, const std::string &program, size_t numPools);

} // namespace dindel
#endif
