// realign_kernel.h — argument block and launcher of the per-read haplotype choice and CIGAR (realign_kernel.hip), shared with launch.cpp.
#ifndef DD_REALIGN_KERNEL_H
#define DD_REALIGN_KERNEL_H
#include "cigar_kernel.h"

namespace ddc {

struct RealignArgs {
    CigarArgs cig;                       /* the walk's inputs; cig.out holds the realign result's n_ops, ops, ref_off and status (per read) */
    int32_t mode;                        /* DD_REALIGN_FIRST_MAX or DD_REALIGN_PAIR */
    int32_t read_begin, read_end;        /* reads this launch covers (the chunks of the host-pointer path) */
    const double *ll;                    /* dd_result.ll */
    const uint8_t *on_hap;               /* dd_result.onHap; NULL = every read is on a haplotype (FIRST_MAX) */
    const int32_t *win_hap_pair;         /* [2 * n_windows] (PAIR) */
    const int32_t *hap_n_indels;         /* [n_haps] (PAIR) */
    int32_t *hap;                        /* dd_realign_result.hap */
};
hipError_t launch_realign(const RealignArgs &A, hipStream_t st);

} // namespace ddc
#endif
