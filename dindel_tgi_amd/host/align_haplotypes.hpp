// align_haplotypes.hpp — DetInDel::alignHaplotypes (reference DInDel.cpp:1427-1524) and the end of getHaplotypes (DInDel.cpp:1600-1626)
// on top of the device alignment (dd_align_haplotypes): the global alignment of every candidate haplotype against its window's
// reference sequence runs on the GPU for a whole batch of windows; what the reference derives from it per window is host work:
//   convertAlignment                          reference ObservationModelSeqAn.hpp:142-269
//   Realign::getFlankingCoordinatesBetter     reference ObservationModelSeqAn.hpp:37-139
//   Haplotype::addRefVariant                  reference Haplotype.hpp:201-251
#ifndef DINDEL_ALIGN_HAPLOTYPES_HPP
#define DINDEL_ALIGN_HAPLOTYPES_HPP
#include <string>
#include <vector>
#include "../../include/dindel_hmm.h"
#include "dindel_types.hpp"
#include "window_io.hpp"

namespace dindel {

// seqan::Dna as a letter: A/a, C/c, G/g, T/t/U/u; every other byte is an A
char dnaLetter(char c);

// flanking coordinates of a variant of `read` (here: the candidate haplotype) against `hapSeq` (here: the window's reference sequence)
void getFlankingCoordinatesBetter(const std::string &hapSeq, size_t readSize, AlignedVariant &av);

// convertAlignment for one haplotype.  refPos: per haplotype base the 0-based offset of the reference base it is paired with, or
// -1 - n when it faces a gap, n = the reference bases left of its column (dd_align_result.ref_pos: the order of a deletion and an
// insertion that touch is part of the alignment, and convertAlignment keys and records them by it).  Fills hap.indels, hap.snps,
// hap.align and hap.refHpos (= ml.hpos); firstBase / lastBase as ml.firstBase / ml.lastBase.
void convertHaplotypeAlignment(const std::string &refSeq, Haplotype &hap, const std::vector<int> &refPos, int *firstBase = NULL, int *lastBase = NULL);

void addRefVariant(Haplotype &hap, int rp);

// One window from its haplotypes' alignments (refPos[h] for w.haps[h]): conversion, the start / end overhang filter and the reference
// variants of alignHaplotypes, then getHaplotypes' removal of duplicate reference haplotypes.  kept (optional): for every haplotype that
// stays, its index in the window as it came in.
void finishWindowHaplotypes(WindowHaplotypes &w, const std::string &refSeq, const std::vector<std::vector<int> > &refPos, std::vector<int> *kept = NULL);

// ---- the variants of an alignment as fixed-size records (dd_hap_variant, include/dindel_hmm.h): csrc/hap_variants_kernel.hip makes them on
//      the device, hapVariantsHost here, word for word the same: the kernel's twin, as blockTableHost is the block table's ----
// Flat arrays as dd_hap_variants_device takes them, host pointers: status and refPos as the alignment left them; summary [n_pairs],
// variants [n_pairs * cap].  Only the records a pair counts are written.
void hapVariantsHost(const dd_align_batch &b, const int32_t *status, const int16_t *refPos, dd_hap_variants_summary *summary, dd_hap_variant *variants, int cap);
// hap.indels, hap.snps and hap.align from a pair's n records (n <= cap), strings formed from the two sequences by position, assigned in
// record order so that a later record of one key replaces an earlier one
void haplotypeFromVariants(const std::string &refSeq, Haplotype &hap, const dd_hap_variant *v, int n);
// hap.refHpos (= ml.hpos) from the slice, a linear walk: hlen = the reference sequence's length
void refHposFromSlice(int hlen, const int16_t *refPos, int rlen, std::vector<int> &refHpos);
// finishWindowHaplotypes from records: summary / variants of the window's haplotypes in order (variants[h * cap ...]).  slices[h]: the
// haplotype's slice or NULL.  A pair flagged DD_HAP_VARIANTS_HOST or with more than cap records goes through convertHaplotypeAlignment and
// needs its slice (std::string thrown without); for the others a slice fills refHpos, and without one refHpos stays empty.
void finishWindowHaplotypesFromVariants(WindowHaplotypes &w, const std::string &refSeq, const dd_hap_variants_summary *summary, const dd_hap_variant *variants,
                                        int cap, const std::vector<const int16_t *> &slices, std::vector<int> *kept = NULL);

// how alignHaplotypesBatch turns the alignments into variants
enum ConvertMode {
    CONVERT_HOST,       // the slice comes back, convertHaplotypeAlignment per haplotype
    CONVERT_DEVICE      // dd_hap_variants_kernel behind the alignment: records and summaries come back; the slice only with needRefHpos, or
                        // (a second alignment call) when a pair needs the host conversion after all
};
const int kHapVariantsCap = 16;       // records per pair of a CONVERT_DEVICE launch

// One device call for all windows' haplotypes (refSeqs[i] belongs to wins[i]), then finishWindowHaplotypes per window.
// Throws std::string: the library's error text, or the first pair the device could not align (an empty or over-long sequence).
// With `errors` a window's own failure (such a pair, or what its conversion throws) is not thrown: errors[i] holds the text, wins[i] is left
// without haplotypes and the other windows are finished; an empty string means the window is done.
// needRefHpos = false (CONVERT_DEVICE only): nobody reads Haplotype::refHpos, it stays empty and the slice stays on the device.
void alignHaplotypesBatch(std::vector<WindowHaplotypes> &wins, const std::vector<std::string> &refSeqs, int device, std::vector<std::string> *errors = NULL,
                          ConvertMode mode = CONVERT_HOST, bool needRefHpos = true);

} // namespace dindel
#endif
