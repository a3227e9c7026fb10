// candidates.hpp — candidate discovery, steps 1 and 2 of the workflow (--analysis getCIGARindels / realignCandidates), on top of the
// device alignment and its indel events (dd_align_haplotypes_events):
//   getIndelFromCIGAR                reference GetCandidates.cpp:64-101
//   alignCIGAR                       reference GetCandidates.cpp:103-195 (the alignment itself is the device's)
//   outputIndels                     reference GetCandidates.cpp:197-258
//   realignCandidateFile             reference GetCandidates.cpp:260-303
//   outputLibraries                  reference GetCandidates.cpp:305-386, collected as in :447-470
//   get / getIndelFromCIGARRegion    reference GetCandidates.cpp:387-486, :50-62
#ifndef DINDEL_CANDIDATES_HPP
#define DINDEL_CANDIDATES_HPP
#include <cstdint>
#ifndef _BACKWARD_BACKWARD_WARNING_H
#define _BACKWARD_BACKWARD_WARNING_H 1       /* <ext/hash_map> is deprecated and announces it; it is used here because the reference uses it */
#endif
#include <ext/hash_map>
#include <iosfwd>
#include <map>
#include <string>
#include <vector>
#include "bam_reader.hpp"
#include "dindel_types.hpp"
#include "glf_to_vcf.hpp"
#include "../../include/dindel_hmm.h"

namespace dindel {

// an indel as a read's CIGAR states it: len > 0 inserted letters (seq), len < 0 deleted bases (seq = that many 'D')
struct CigarIndel {
    uint32_t refpos; int len; std::string seq;
    CigarIndel(uint32_t p, int l, const std::string &s) : refpos(p), len(l), seq(s) {}
    bool operator<(const CigarIndel &o) const        // GetCandidates.hpp:70-73: position, then sequence, then length
    {
        if (refpos != o.refpos) return refpos < o.refpos;
        return seq != o.seq ? seq < o.seq : len < o.len;
    }
};

// The I and D operations of one record.  Throws std::string("I don't know how to smoke this CIGAR") at P, = and X.
void cigarIndels(const RawBamView &rec, std::vector<CigarIndel> &out);

// position -> candidates with their read counts.  The reference keeps this in a __gnu_cxx::hash_map and walks it in the container's
// order; behind the realignment a variant's count is assigned, not summed, so when two candidates land on one canonical variant the
// later one in that order wins.  The same container with the same insertion sequence gives the same order by construction.
typedef __gnu_cxx::hash_map<int, std::map<CigarIndel, int> > CandidateTable;
void addCandidate(CandidateTable &t, const CigarIndel &id);
// the order in which a __gnu_cxx::hash_map<int, ...> that received `keys` in this sequence (repeats allowed) is walked
inline std::vector<int> hashMapOrder(const std::vector<int> &keys)
{
    __gnu_cxx::hash_map<int, int> m;
    for (size_t i = 0; i < keys.size(); i++) m[keys[i]] = 1;
    std::vector<int> order;
    for (__gnu_cxx::hash_map<int, int>::const_iterator it = m.begin(); it != m.end(); ++it) order.push_back(it->first);
    return order;
}

// The indel events of one alignment from its slice of reference offsets (dd_align_result.ref_pos), by the rules of dd_align_events: what
// the device kernel computes, on the host — for pairs whose events exceed the cap, and for alignments that did not come from the device.
void alignmentEvents(const int16_t *refPos, int hapLen, int refLen, std::vector<dd_align_events> &out);

// In place of the device (tests; any other aligner): fills status [n_pairs] and the slices (laid out like b->hap_seq) of a host batch.
typedef void (*AlignHook)(void *data, const dd_align_batch *b, int32_t *status, int16_t *refPos);

struct CandidateOptions {
    int device, batchCandidates, eventsCap;
    bool hostConvert, quiet;
    AlignHook hook; void *hookData;
    CandidateOptions() : device(0), batchCandidates(65536), eventsCap(8), hostConvert(false), quiet(false), hook(NULL), hookData(NULL) {}
};
struct CandidateStats {
    long candidates, dropped, tooLong, overflowed, batches;
    CandidateStats() : candidates(0), dropped(0), tooLong(0), overflowed(0), batches(0) {}
};

// samtools' fai_fetch as Fasta::getSequence uses it: [begin1, end1] one-based and inclusive, begin clamped to 1, end to the target's
// length, upper-cased; empty for an unknown target or nothing left
std::string fetchReference(IndexedFasta &fa, const std::string &tid, long begin1, long end1);

// Realign every candidate of one target and write its lines: `tid pos variant ... # count ...`, positions ascending
void outputIndels(const std::string &tid, const CandidateTable &table, std::ostream &out, IndexedFasta &fa, const CandidateOptions &opt,
                  CandidateStats &stats);

// library name -> |insert size| -> pairs, sizes in a hash_map as in the reference (its walk orders the terms of mean and variance)
typedef __gnu_cxx::hash_map<int, long> InsertSizes;
typedef std::map<std::string, InsertSizes> LibraryInsertSizes;
void outputLibraries(LibraryInsertSizes &libs, std::ostream &out, bool quiet);

// the three flows; all throw std::string
void candidatesFromBam(const std::string &bamFile, const std::string &outputFile, IndexedFasta &fa, const CandidateOptions &opt, CandidateStats &stats);
void candidatesFromRegion(const std::vector<std::string> &bamFiles, const std::string &tid, int start, int end, const std::string &outputFile,
                          IndexedFasta &fa, const CandidateOptions &opt, CandidateStats &stats);
void realignCandidateFile(const std::string &varFile, bool isOneBased, const std::string &outputFile, IndexedFasta &fa,
                          const CandidateOptions &opt, CandidateStats &stats);

// --region "A-B" (commas allowed in the numbers) -> [start, end); throws std::string (reference DInDel.cpp:3892-3905)
void parseRegion(const std::string &region, int &start, int &end);

// the tool (host/dindel_candidates.cpp is this call); hook as in CandidateOptions
int candidatesMain(int argc, char **argv, AlignHook hook, void *hookData);

} // namespace dindel
#endif
