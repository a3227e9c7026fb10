// haplotypes.hpp — the first two parts of DetInDel::getHaplotypes (reference DInDel.cpp:1526-1592): the empirical haplotype distribution
// of a window's reads and the candidate sequences made from it.
//   HaplotypeDistribution (constructor, insertRead, insertSeq, setFrequencies)   reference HaplotypeDistribution.cpp:29-45, 74-164, 179-436
//   HapBlock                                                                      reference HapBlock.cpp:20-81
//   HDIterator2 (setupBlocks, setThresholds, generateHapsWithAlignedVariants)     reference HaplotypeDistribution.hpp:85-116, 171-309, 312-482
// The distribution is not built by inserting and splitting one segment at a time: its end state inside the window has a closed form
// (csrc/hapdist_kernel.hip computes it on the device, blockTableHost here on the host, both into the flat tables of dd_hap_blocks), and a
// window the closed form does not cover goes through sequentialTable, which replays the segments in order.  Written from the behaviour.
#ifndef DINDEL_HAPLOTYPES_HPP
#define DINDEL_HAPLOTYPES_HPP
#include <string>
#include <vector>
#include "../../include/dindel_hmm.h"
#include "dindel_types.hpp"

namespace dindel {

class IndexedFasta;

// one string of a block with what setFrequencies leaves on it
struct BlockEntry { std::string seq; int count; bool isRef; double freq; };
// a block: [start, end] on the reference; an insertion block sits in front of `start` and has end = start - 1 once selected
struct HapBlockTable { uint32_t start, end; bool insertion; std::vector<BlockEntry> entries; };
// what selectBlocks needs of a window's distribution: the blocks inside [rs, re] in order, the insertion blocks inside it by position,
// and `left` as in dd_hap_blocks
struct WindowTable { std::vector<HapBlockTable> blocks, insertions; int left; };

// the reads of a batch of windows as the block table wants them; batch() views the vectors (which must stay alive and unchanged)
struct HapBatchData {
    std::vector<int32_t> winRs, winRefOff, winReadOff, readPos, readFlag, readOpOff, readBaseOff;
    std::vector<uint32_t> ops;
    std::string refSeq, bases;
    HapBatchData() : winRefOff(1, 0), winReadOff(1, 0), readOpOff(1, 0), readBaseOff(1, 0) {}
    void addWindow(int32_t rs, const std::string &ref) { winRs.push_back(rs); refSeq += ref; winRefOff.push_back(int32_t(refSeq.size())); winReadOff.push_back(winReadOff.back()); }
    // a read of the window added last
    void addRead(int32_t pos, int32_t flag, const uint32_t *cigar, size_t nCigar, const std::string &letters);
    int nWindows() const { return int(winRs.size()); }
    dd_hap_batch batch() const;
};
// the tables of a batch with the capacities of dd_hap_blocks_offsets; tables() views the vectors
struct HapTablesData {
    std::vector<int32_t> perWindow, blkOff, entOff, insOff;
    std::vector<uint32_t> blocks, entries, insOps, insPos;
    void size(const dd_hap_batch &b);          // throws std::string
    dd_hap_blocks tables();
};

// The closed form on flat arrays: the kernel's twin, statuses included (a window that is not DD_HAPDIST_OK has only its status written).
void blockTableHost(const dd_hap_batch &b, dd_hap_blocks &t);
// an OK window of the flat tables as a WindowTable, frequencies set
WindowTable tableFromFlat(const dd_hap_batch &b, const dd_hap_blocks &t, int w);
// The fallback for every other window: the segments one after the other, in the reference's order, on blocks of any length that are
// split where a segment begins or ends.  Throws the reference's strings ("Mag niet.", "I don't know how to smoke this CIGAR").
WindowTable sequentialTable(const dd_hap_batch &b, int w);

// HDIterator2::setupBlocks: the blocks wholly inside [left, right], insertion blocks placed as the reference's list walk places them.
// Throws "Blocks are not consecutive." and "Not enough blocks.".
std::vector<HapBlockTable> selectBlocks(const WindowTable &t, uint32_t rs, uint32_t left, uint32_t right);
// HDIterator2::setThresholds: drops the rarest non-reference strings until at most maxHap combinations are left; returns logNumHap.
// Throws "Cannot find reference sequence.".
double setThresholds(std::vector<HapBlockTable> &hbs, size_t maxHap);
// HDIterator2::generateHapsWithAlignedVariants: the combinations, deletions carried out, the window's variants added; ordered by sequence.
// Throws "What's going on here?".
std::vector<std::string> generateHaplotypes(const std::vector<HapBlockTable> &hbs, const std::vector<AlignedVariant> &variants, bool changeINStoN);

struct HaplotypeOptions {
    HaplotypeOptions() : maxHap(8), skipMaxHap(200), maxHapReadProd(10000000.0), changeINStoN(false), hostDistribution(false), device(0) {}
    size_t maxHap, skipMaxHap; double maxHapReadProd; bool changeINStoN, hostDistribution; int device;
};
struct WindowCandidates {
    uint32_t leftPos, rightPos;                // in: the window's; out: the selected blocks' bounds (hdi.start() / hdi.end())
    std::vector<AlignedVariant> variants;
    size_t nReads;
    std::vector<std::string> haps;             // out
    std::string message;                       // out: empty, or why the window has no haplotypes (the reference's text)
    // out, with a message: getHaplotypes RETURNED true (DInDel.cpp:1569 / :1581: a cerr line, nothing thrown) with this many haplotypes
    // made (0 at :1569); false: `message` is a thrown string, which the window loop turns into the window's skipped line
    bool returnedSkip; size_t hapsAtSkip;
    WindowCandidates() : leftPos(0), rightPos(0), nReads(0), returnedSkip(false), hapsAtSkip(0) {}
};
// one window from its table: selectBlocks, setThresholds, the two skip tests of DInDel.cpp:1569 / :1581, generateHaplotypes
void haplotypesFromTable(const WindowTable &t, uint32_t rs, const HaplotypeOptions &opt, WindowCandidates &win);
// a batch: one device call (or blockTableHost with opt.hostDistribution), sequentialTable for the windows that are not OK, then the host
// steps per window.  stats, if given: {windows OK on the table path, windows through sequentialTable}.  Throws std::string on a library error.
void getHaplotypesBatch(const HapBatchData &data, std::vector<WindowCandidates> &wins, const HaplotypeOptions &opt, size_t stats[2] = 0);

// what the tool and the window loop's haplotype stage (dindel_gpu --ref) share (host/haplotypes_main.cpp):
// getRefSeq(first1, last1) of the reference: 1-based, inclusive, cut at the sequence's end, letters as the file has them
std::string refPiece(IndexedFasta &fa, const std::string &tid, long first1, long last1);
// the selected reads of the window added last, from their records (ReadSelectionParameters::keepRecords): CIGAR, flag, raw letters
void addWindowReads(HapBatchData &data, const std::vector<Read> &reads);

// the tool (host/dindel_haplotypes.cpp)
int haplotypesMain(int argc, char **argv);

} // namespace dindel
#endif
