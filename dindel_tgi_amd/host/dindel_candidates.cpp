// dindel_candidates — steps 1 and 2 of the workflow (--analysis getCIGARindels / realignCandidates of the reference's main,
// DInDel.cpp:4236-4294) as a tool: candidate indels from the CIGARs of a BAM file (with the libraries' insert-size histograms) or from a
// candidate file, each realigned to its canonical position by the global alignment on the GPU.  Everything is host/candidates.cpp.
//
//   dindel_candidates --analysis getCIGARindels --bamFile IN.bam --ref REF.fa --outputFile OUT
//   dindel_candidates --analysis realignCandidates --varFile IN.variants.txt --ref REF.fa --outputFile OUT
#include "candidates.hpp"

int main(int argc, char **argv) { return dindel::candidatesMain(argc, argv, NULL, NULL); }
