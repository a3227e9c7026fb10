// pooled_em_kernel.h — argument block and launcher of the pooled analysis' EM kernel (pooled_em_kernel.hip), and what its entry points
// (pooled_em_capi.cpp) share with the host evaluation (pooled_em_host.cpp).
#ifndef DD_POOLED_EM_KERNEL_H
#define DD_POOLED_EM_KERNEL_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dindel_hmm.h"

namespace ddp {

struct PooledEmArgs {
    int32_t n_windows, max_haps;         // max_haps: what the launch's LDS was sized for; a slot with more haplotypes gets iters = -1
    int64_t n_slots;
    const int32_t *win_hap_off, *win_read_off;
    const int64_t *win_pair_off;
    const double *ll;                    // per pair, liks[h][r] order
    dd_pooled_slots s;
    dd_pooled_result out;
    double a0, tol;
};

// LDS of one workgroup (one wavefront, one slot): per-lane counts nk[h][lane], then lpi, pi and the counts' totals per haplotype
inline size_t pooled_em_lds_bytes(int max_haps) { return (size_t)(max_haps > 0 ? max_haps : 1) * (64 + 3) * sizeof(double); }
hipError_t launch_pooled_em(const PooledEmArgs &A, hipStream_t st);

} // namespace ddp

namespace ddh {
// pooled_em_host.cpp: a batch's slot tables and outputs checked (host pointers); max_haps_out: the most haplotypes a slot has
int check_pooled_slots(const dd_batch *b, const dd_pooled_slots *s, double a0, double tol, const dd_pooled_result *out, int *max_haps_out);
}
#endif
