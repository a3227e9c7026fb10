// hap_variants_kernel.h — argument block and launcher of the variant extraction (hap_variants_kernel.hip), shared with align_host.cpp.
#ifndef DD_HAP_VARIANTS_KERNEL_H
#define DD_HAP_VARIANTS_KERNEL_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hapalign_kernel.h"

namespace dda {

/* The variants launch runs behind an alignment launch and keeps its three words DD_VARIANTS_HDR_* in that launch's workspace header
 * (draw_header.h): zeroed on the stream in front of the variants launch. */

struct VariantsArgs {
    int32_t n_refs, n_pairs;
    const int32_t *ref_off;              /* [n_refs + 1] */
    const uint8_t *ref_seq;              /* raw letters: the flanks compare them as they are, variants and SNPs their seqan::Dna letters */
    const int32_t *pair_ref, *hap_off;   /* [n_pairs], [n_pairs + 1] */
    const uint8_t *hap_seq;
    const int32_t *status;               /* [n_pairs] as the alignment left it */
    const int16_t *ref_pos;              /* laid out like hap_seq */
    dd_hap_variants_summary *summary;    /* [n_pairs] */
    dd_hap_variant *variants;            /* [n_pairs * cap] */
    int32_t cap;
    unsigned int *hdr;                   /* the alignment workspace's header, as u32 words */
};

hipError_t launch_hap_variants(const VariantsArgs &A, hipStream_t st);

} // namespace dda
#endif
