// pooled_em_kernel.hip — the EM loop of the pooled analysis (estimateHaplotypeFrequenciesBayesEM, reference DInDel.cpp:2412-2543) on the `ll`
// array the likelihood kernels leave in HBM.
//
// One wavefront (one workgroup) per slot = (window, set of active variants).  The lanes take the window's reads r = lane, lane + 64, ...
// (rl[h * R + r]: neighbouring lanes load neighbouring doubles), each keeps its own partial sums — the counts nk[h] in LDS laid out
// [h][lane], S and the log-likelihood in registers — and the partials are combined x[i] += x[i + off], off = 32 ... 1.  That is the one
// summation order of pooled_math.h, whose functions are the only arithmetic here: every output is bit-equal to dd_pooled_em_host.
// No atomics; the LDS is sized from the batch's largest haplotype count (4 KB at 8 haplotypes, 105 KB at 200), one code path for all.
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>
#include "kernel_common.h"
#include "pooled_em_kernel.h"
#include "pooled_math.h"

namespace ddp {

// lane 0's value is the sum in pooled_math.h's order (PmSerialSum::total); it is handed to every lane
__device__ __forceinline__ double wave_total(double x)
{
#pragma unroll
    for (int off = PM_LANES / 2; off >= 1; off >>= 1) x = x + __shfl_down(x, off);
    return __shfl(x, 0);
}

__global__ void __launch_bounds__(64) dd_pooled_em_kernel(PooledEmArgs P)
{
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int64_t slot = blockIdx.x;
    if (slot >= P.n_slots) return;
    const int w = P.s.slot_window[slot];
    const int64_t so = P.s.slot_off[slot];
    int H = -1, R = 0;
    if (w >= 0 && w < P.n_windows) { H = P.win_hap_off[w + 1] - P.win_hap_off[w]; R = P.win_read_off[w + 1] - P.win_read_off[w]; }
    if (H < 0 || H > P.max_haps || R < 0 || P.s.slot_off[slot + 1] - so != H) {     // tables that do not fit each other: nothing is read
        if (lane == 0) { P.out.iters[slot] = -1; P.out.loglik[slot] = 0.0; P.out.ediff[slot] = 0.0; }
        return;
    }
    const double *rl = P.ll + P.win_pair_off[w];
    const uint8_t *compat = P.s.compat + so;
    double *nk = lds, *lpi = lds + (size_t)64 * P.max_haps, *pi = lpi + P.max_haps, *nk_tot = pi + P.max_haps;
    const double a0 = P.a0, tol = P.tol;

    int numah = 0;
    for (int h = 0; h < H; h++) numah += compat[h] != 0;
    const double lpi0 = numah ? pm_log(1.0 / (double)numah) : 0.0;
    for (int h = lane; h < H; h += 64) lpi[h] = compat[h] ? lpi0 : PM_INCOMPATIBLE;
    __syncthreads();
    const double denom = (double)numah * a0 + (double)R;
    double eOld = -pm_inf(), loglik = 0.0, ediff = 0.0;
    int iter = 0;
    bool converged = false;
    while (!converged) {
        for (int h = 0; h < H; h++) nk[h * 64 + lane] = 0.0;
        double S = 0.0, L = 0.0;
        for (int r = lane; r < R; r += 64) {
            double lognorm = -pm_inf();
            for (int h = 0; h < H; h++) lognorm = pm_add_logs(lognorm, lpi[h] + rl[(int64_t)h * R + r]);
            for (int h = 0; h < H; h++) {
                const double v = rl[(int64_t)h * R + r], z = pm_exp((lpi[h] + v) - lognorm);
                nk[h * 64 + lane] = nk[h * 64 + lane] + z;
                S = S + z * v;
            }
            L = L + lognorm;
        }
        loglik = wave_total(L);
        double eNew = wave_total(S);
        for (int h = 0; h < H; h++) {
            const double t = wave_total(nk[h * 64 + lane]);
            if (lane == 0) nk_tot[h] = t;
        }
        __syncthreads();
        double ahat = 0.0;
        for (int h = 0; h < H; h++)
            if (compat[h]) ahat = ahat + (nk_tot[h] + a0);
        const double dahat = numah ? pm_digamma(ahat) : 0.0;
        for (int h = lane; h < H; h += 64) pm_m_step(compat[h] != 0, nk_tot[h], a0, dahat, denom, lpi[h], pi[h]);
        __syncthreads();
        for (int h = 0; h < H; h++) eNew = eNew + pi[h] * nk_tot[h];
        ediff = pm_abs(eOld - eNew);
        converged = ediff < tol || iter > PM_MAX_ITER;
        eOld = eNew;
        iter++;
        __syncthreads();                 // nk_tot and lpi are rewritten by the next iteration
    }
    double zsum = 0.0;
    for (int h = 0; h < H; h++) zsum = zsum + pm_exp(pi[h]);
    for (int h = lane; h < H; h += 64) P.out.freqs[so + h] = pm_exp(pi[h]) / zsum;
    if (lane == 0) { P.out.loglik[slot] = loglik; P.out.iters[slot] = iter; P.out.ediff[slot] = ediff; }
}

hipError_t launch_pooled_em(const PooledEmArgs &A, hipStream_t st)
{
    if (A.n_slots <= 0) return hipSuccess;
    if (A.max_haps < 0 || pooled_em_lds_bytes(A.max_haps) > 160u * 1024u) return hipErrorInvalidValue;   // one workgroup cannot hold more than the CU's LDS
    static std::atomic<unsigned> raised{0};
    hipError_t e = ddc::raise_lds_cap_once(reinterpret_cast<const void *>(dd_pooled_em_kernel), raised);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dd_pooled_em_kernel, dim3((unsigned)A.n_slots), dim3(64), pooled_em_lds_bytes(A.max_haps), st, A);
    return hipGetLastError();
}

} // namespace ddp
