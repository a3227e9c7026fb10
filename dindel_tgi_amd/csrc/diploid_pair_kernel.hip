// diploid_pair_kernel.hip — the window's MAP haplotype pair, chosen and certified on the `ll` the likelihood kernels leave in HBM
// (diploid_pair_kernel.h holds the definition and every piece of arithmetic; the CPU evaluation is diploid_pair_host.cpp).
//
// One wavefront (one workgroup) per window, the workgroups of a persistent grid striding over the windows.  A window's pairs h1 <= h2 are
// taken 64 at a time, one per LANE: a lane adds its pair's terms in read order (dp_acc_add), so the order of every sum is the host's and no
// value crosses lanes until the sums are done.  Lanes that share a haplotype read the same row of ll, so the rows go through LDS in chunks
// of kReadChunk reads of every haplotype (rows padded by one double: lanes of different h1 fall on different banks).  Each lane keeps the two
// first pairs it has seen in the order (V descending, index ascending); that order has no ties, so merging the lanes' records by xor
// shuffles gives every lane the window's two first pairs whatever the merge order.  Lane 0 writes the window's outputs with ordinary
// vector stores.  A pass over the window's status and ll in front finds the states in which no sum is taken.  No max instruction, no
// atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "diploid_pair_kernel.h"

namespace ddq {

constexpr int kRow = kReadChunk + 1;

__device__ __forceinline__ void wave_merge(DpTop2 &t)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        DpTop2 o;
        o.v1 = __shfl_xor(t.v1, off); o.e1 = __shfl_xor(t.e1, off); o.p1 = __shfl_xor(t.p1, off);
        o.v2 = __shfl_xor(t.v2, off); o.e2 = __shfl_xor(t.e2, off); o.p2 = __shfl_xor(t.p2, off);
        dp_top2_merge(t, o);
    }
}

__global__ void __launch_bounds__(64) dd_diploid_pair_kernel(DiploidPairArgs P)
{
    __shared__ double rows[DD_DIPPAIR_MAX_HAPS * kRow];
    const int lane = threadIdx.x;
    const double log_half = pm_log(0.5);
    for (int w = blockIdx.x; w < P.n_windows; w += gridDim.x) {
        const int H = P.win_hap_off[w + 1] - P.win_hap_off[w];
        int R = P.win_read_off[w + 1] - P.win_read_off[w];
        if (R < 0) R = 0;
        const double *ll = P.ll + P.win_pair_off[w];
        int early = DD_DIPPAIR_CERTIFIED;
        if (H <= 0) {
            early = DD_DIPPAIR_NO_HAPS;
        } else if (H > DD_DIPPAIR_MAX_HAPS) {
            early = DD_DIPPAIR_TOO_MANY_HAPS;
        } else {
            const int32_t *status = P.status ? P.status + P.win_pair_off[w] : nullptr;
            const int64_t n = (int64_t)H * R;
            bool bad_status = false, bad_ll = false;
            for (int64_t i = lane; i < n; i += 64) {
                if (status && status[i] != 0) bad_status = true;
                if (!dp_finite(ll[i])) bad_ll = true;
            }
            if (__any(bad_status)) early = DD_DIPPAIR_NOT_COMPUTED;
            else if (__any(bad_ll)) early = DD_DIPPAIR_NONFINITE;
        }
        DpTop2 top;
        dp_top2_clear(top);
        bool nan_v = false;
        if (early == DD_DIPPAIR_CERTIFIED) {                           // wave-uniform
            const double *prior = P.prior + P.win_hh_off[w];
            const int n_pairs = H * (H + 1) / 2;
            for (int p0 = 0; p0 < n_pairs; p0 += 64) {
                const int p = p0 + lane;
                const bool live = p < n_pairs;
                int h1 = 0, h2 = 0;
                if (live) dp_pair_of_index(H, p, h1, h2);
                DpAcc acc;
                dp_acc_clear(acc);
                for (int r0 = 0; r0 < R; r0 += kReadChunk) {
                    const int nr = R - r0 < kReadChunk ? R - r0 : kReadChunk;
                    __syncthreads();                                   // the chunk before this one has been read
                    for (int i = lane; i < H * kReadChunk; i += 64) {
                        const int h = i / kReadChunk, rr = i % kReadChunk;
                        if (rr < nr) rows[h * kRow + rr] = ll[(int64_t)h * R + r0 + rr];
                    }
                    __syncthreads();
                    if (live)
                        for (int rr = 0; rr < nr; rr++) dp_acc_add(acc, rows[h1 * kRow + rr], rows[h2 * kRow + rr], log_half);
                }
                if (live) {
                    double V, eps;
                    dp_value(acc, R, prior[(int64_t)h1 * H + h2], V, eps);
                    if (V != V) nan_v = true;
                    dp_top2_offer(top, V, eps, p);
                }
            }
            wave_merge(top);
        }
        const bool any_nan = __any(nan_v);
        if (lane == 0)
            dp_finish(H, early, any_nan, top, P.out.pair + 2 * (int64_t)w, P.out.state + w, P.out.best + w, P.out.gap + w, P.out.margin + w);
    }
}

hipError_t launch_diploid_pairs(const DiploidPairArgs &A, hipStream_t st)
{
    if (A.n_windows <= 0) return hipSuccess;
    const int blocks = A.n_windows < kMaxBlocks ? A.n_windows : kMaxBlocks;
    hipLaunchKernelGGL(dd_diploid_pair_kernel, dim3((unsigned)blocks), dim3(64), 0, st, A);
    return hipGetLastError();
}

} // namespace ddq
