// dindel_pooled2glf — the per-pool genotype likelihoods of the called sites (the reference's `python makeGenotypeLikelihoodFilePooled.py`)
// as a tool.  Everything is host/pooled_vcf.cpp; no GPU.
//
//   dindel_pooled2glf -g LIST_OF_GLF_FILES.txt -c CALLS.vcf -o CALLED.glf.txt -b POOLS.txt
#include "pooled_vcf.hpp"

int main(int argc, char **argv) { return dindel::pooledGlfMain(argc, argv); }
