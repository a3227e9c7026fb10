// dindel_pooled2vcf — the calls of the pooled workflow (the reference's `python mergeOutputPooled.py`) as a tool: the `singlevariant`
// lines of dindel_gpu --doPooled -> a VCF.  Everything is host/pooled_vcf.cpp; no GPU.
//
//   dindel_gpu --doPooled --bamFiles POOLS.txt ... --outputFile PREFIX
//   dindel_pooled2vcf -i LIST_OF_GLF_FILES.txt -o CALLS.vcf -r REF.fa --numSamples N --numBamFiles P [--filterFR] [--filterQual 20] [--maxHPLen 10]
#include "pooled_vcf.hpp"

int main(int argc, char **argv) { return dindel::pooledVcfMain(argc, argv); }
