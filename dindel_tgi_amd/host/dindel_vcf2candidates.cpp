// dindel_vcf2candidates — candidates that do not come from the sample's own CIGARs (the reference's `python convertVCFToDindel.py`) as a
// tool: a VCF of known indels -> `tid pos variant` lines.  Everything is host/vcf_candidates.cpp; no GPU.
//
//   dindel_vcf2candidates -i SITES.vcf[,MORE.vcf.gz] -o KNOWN.variants.txt -r REF.fa [--minQual 1] [--tid NAME --region A-B]
//   dindel_candidates --analysis realignCandidates --varFile KNOWN.variants.txt --ref REF.fa --outputFile KNOWN.realigned
#include "vcf_candidates.hpp"

int main(int argc, char **argv) { return dindel::vcfCandidatesMain(argc, argv); }
