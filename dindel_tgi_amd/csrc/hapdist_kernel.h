// hapdist_kernel.h — argument block and launcher of the block-table kernel (hapdist_kernel.hip), shared with hapdist_host.cpp.
#ifndef DD_HAPDIST_KERNEL_H
#define DD_HAPDIST_KERNEL_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dindel_hmm.h"
#include "draw_header.h"

namespace dda {

#define DD_HAPDIST_WAVES 4            /* wavefronts per workgroup, one window each */
#define DD_HAPDIST_MAX_BLOCKS 512     /* workgroups of the persistent grid: two per CU */
#define DD_HAPDIST_WS_BYTES 256       /* the workspace: a header of u32 words, of which the launch uses DD_HAPDIST_HDR_* (draw_header.h) */

struct HapdistArgs {
    dd_hap_batch b;
    dd_hap_blocks t;
    int64_t max_blk, max_ent, max_ins;
    unsigned int *hdr;
};

hipError_t launch_hapdist(const HapdistArgs &A, hipStream_t st);

} // namespace dda
#endif
