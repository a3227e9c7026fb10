// realigned_bam.hpp — "next" row N4, the output half: --outputRealignedBAM of the diploid analysis.
//   the haplotype pair and, per read, the haplotype whose alignment is written     reference DInDel.cpp:589-612
//   computePairLikelihoods (usePrior) + getMaxHap                                  reference DInDel.cpp:3765-3833, :290-318
//   writeRealignedBAMFile                                                          reference DInDel.cpp:670-725
// getCIGAR itself is host/cigar.cpp.  The BAM is written by the own BGZF writer (bam_reader.hpp); libbam is not in the image.
#ifndef DINDEL_REALIGNED_BAM_HPP
#define DINDEL_REALIGNED_BAM_HPP
#include <functional>
#include <string>
#include <vector>
#include "bam_reader.hpp"
#include "cigar.hpp"
#include "compute_likelihoods.hpp"
#include "diploid_glf.hpp"

namespace dindel {

// The most likely haplotype pair with priors (the head of computePairLikelihoods' sorted list, which is what getMaxHap returns).
// All pairs take part: filterHaplotypes plays no role here.  Throws std::string if no pair has a finite likelihood.
std::pair<int, int> maxLikelihoodPair(const std::vector<Haplotype> &haps, const std::vector<Read> &reads, const WindowLikelihoods &liks,
                                      int leftPos, const AlignedCandidates &candidateVariants, const DiploidParameters &params);
// Its sums and argmax over lh haplotypes and numReads reads, with the likelihoods and the pair priors as functions (maxLikelihoodPair hands
// over the window's and getHaplotypePrior).  values (may be NULL): every pair's likelihood with prior at [hp * lh + hm], hp <= hm.
std::pair<int, int> maxLikelihoodPairOf(size_t lh, size_t numReads, const std::function<double(size_t, size_t)> &ll,
                                        const std::function<double(size_t, size_t)> &prior, std::vector<double> *values);

// One CIGAR per read against haplotype h1 or h2 of the pair, whichever explains the read better (within 1e-8: the one with fewer
// indels, h2 on a tie) — DInDel.cpp:596-611.  Needs Haplotype::refHpos and the reads' alignments (a batch run with alignments).
// Throws getCIGAR's strings.
void realignedCigars(const std::vector<Haplotype> &haps, const std::vector<Read> &reads, const WindowLikelihoods &liks, std::pair<int, int> pair,
                     int refSeqPos, std::vector<CIGAR> &cigars);

// The same with device CIGARs (LikelihoodEngine::setDeviceCigars, liks.hasDeviceCigars()): the haplotype of the pair is picked per read
// exactly as above, and the read's CIGAR is the one the device computed for that (haplotype, read) pair.  A status that names a throw
// raises the string getCIGAR throws there.  A read whose CIGAR has more operations than the batch's cap (DD_CIGAR_OVERFLOW) is redone
// with getCIGAR on the host from `withAlignments()` — the same window computed with its per-base alignments, asked for at most once per
// call — and counted in *hostFallbacks.  Without device CIGARs in `liks` this is the function above.
void realignedCigars(const std::vector<Haplotype> &haps, const std::vector<Read> &reads, const WindowLikelihoods &liks, std::pair<int, int> pair,
                     int refSeqPos, std::vector<CIGAR> &cigars, const std::function<WindowLikelihoods()> &withAlignments, long *hostFallbacks);

// The pooled analysis' own choice (DInDel.cpp:498-520): a read placed on a haplotype (onHap) is realigned to the FIRST haplotype with the
// largest ll — strict `>` from -HUGE_VAL, so index 0 when none compares greater (all -inf, NaN), DInDel.cpp:503-512 — and gets getCIGAR's
// CIGAR against it; a read without onHap keeps an empty CIGAR, and writeRealignedBAMFile copies its record.  Throws getCIGAR's strings.
void pooledRealignedCigars(const std::vector<Haplotype> &haps, const std::vector<Read> &reads, const WindowLikelihoods &liks, int refSeqPos,
                           std::vector<CIGAR> &cigars);
// The same with device CIGARs, exactly as the second realignedCigars above uses them: the same status-to-throw mapping, a read over the
// batch's cap redone on the host from `withAlignments()` and counted in *hostFallbacks.  Without device CIGARs in `liks`: the function above.
void pooledRealignedCigars(const std::vector<Haplotype> &haps, const std::vector<Read> &reads, const WindowLikelihoods &liks, int refSeqPos,
                           std::vector<CIGAR> &cigars, const std::function<WindowLikelihoods()> &withAlignments, long *hostFallbacks);
// The same from the realigned reads the device chose (LikelihoodEngine::setDeviceRealign, liks.hasDeviceRealign(); the function above calls
// this for such a view): reads in order, haplotype liks.realignHap(r) and its CIGAR straight from the view.  DD_REALIGN_OFF_HAP (and a
// window without haplotypes) leaves the empty CIGAR, a throw code raises getCIGAR's string, DD_CIGAR_OVERFLOW and DD_CIGAR_NOT_COMPUTED are
// redone with getCIGAR for that haplotype from `withAlignments()` and counted in *hostFallbacks — the status table and the fallback are
// the ones of the per-pair device CIGARs.  Nothing of the choice is restated here.
void pooledDeviceRealignedCigars(const std::vector<Haplotype> &haps, const std::vector<Read> &reads, const WindowLikelihoods &liks, int refSeqPos,
                                 std::vector<CIGAR> &cigars, const std::function<WindowLikelihoods()> &withAlignments, long *hostFallbacks);
// What both are made of: the choice per read from ll(h, r) and onHap(r), the CIGAR of the chosen pair from cigarOf(h, r).
void pooledRealignedCigars(size_t numHaps, size_t numReads, const std::function<double(size_t, size_t)> &ll, const std::function<bool(size_t)> &onHap,
                           const std::function<CIGAR(size_t, size_t)> &cigarOf, std::vector<CIGAR> &cigars);

// --deviceRealignDiploid: the diploid step's CIGARs from a view with hasDevicePair().  On a window the device certified (pairState() ==
// DD_DIPPAIR_CERTIFIED) the pair is devicePair() and each read's CIGAR the row of its realignHap(r) — nothing of the pair choice is computed
// here; rows over the cap or not computed go through the host getCIGAR from withAlignments(), counted in *hostFallbacks.  On any other state
// the window is the host's: maxLikelihoodPair, then realignedCigars on withAlignments(); *uncertifiedWindows is incremented.  Returns the pair used.
std::pair<int, int> diploidDeviceRealignedCigars(const std::vector<Haplotype> &haps, const std::vector<Read> &reads, const WindowLikelihoods &liks, int leftPos,
                                                 const AlignedCandidates &candidateVariants, const DiploidParameters &params, int refSeqPos,
                                                 std::vector<CIGAR> &cigars, const std::function<WindowLikelihoods()> &withAlignments, long *hostFallbacks,
                                                 long *uncertifiedWindows);

// The name the reference gives the window's file: PREFIX.ra.INDEX_TID_(leftPos+minReadOverlap)_(rightPos-minReadOverlap).bam (:614-618)
std::string realignedBAMFileName(const std::string &prefix, int index, const std::string &tid, uint32_t leftPos, uint32_t rightPos, int minReadOverlap);

// writeRealignedBAMFile: every read of the window in `reads` order; a read placed on a haplotype (onHap) gets its new CIGAR,
// position = cigar.refPos and isize = refPos - mpos (bin and everything else as in the original record); the others are copied.
// Throws "Problem with the cigars.", "Cannot open bamfile ... for writing!"; a read without its record: "Read has no BAM record."
void writeRealignedBAMFile(const std::string &fileName, const std::vector<CIGAR> &cigars, const std::vector<Read> &reads, const std::vector<int> &onHap,
                           const BamFile &header);

} // namespace dindel
#endif
