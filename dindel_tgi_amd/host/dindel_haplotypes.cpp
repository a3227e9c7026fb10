// dindel_haplotypes — the first two parts of DetInDel::getHaplotypes (reference DInDel.cpp:1526-1592) as a tool: the empirical haplotype
// distribution of every window's reads (its block table on the GPU, csrc/hapdist_kernel.hip) and the candidate haplotypes made from it
// and from the window's candidate variants.  Everything is host/haplotypes.cpp and host/haplotypes_main.cpp.
//
//   dindel_haplotypes --bamFile IN.bam --ref REF.fa --varFile WINDOWS.txt --outputFile OUT.haps.txt
//   dindel_hapalign --hapFile OUT.haps.txt --outputFile OUT.aligned.txt
#include "haplotypes.hpp"

int main(int argc, char **argv) { return dindel::haplotypesMain(argc, argv); }
