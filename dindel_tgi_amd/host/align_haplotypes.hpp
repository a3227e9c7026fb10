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

// One device call for all windows' haplotypes (refSeqs[i] belongs to wins[i]), then finishWindowHaplotypes per window.
// Throws std::string: the library's error text, or the first pair the device could not align (an empty or over-long sequence).
void alignHaplotypesBatch(std::vector<WindowHaplotypes> &wins, const std::vector<std::string> &refSeqs, int device);

} // namespace dindel
#endif
