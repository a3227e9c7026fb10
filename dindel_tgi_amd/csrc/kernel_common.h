// kernel_common.h — what the kernel files share besides their argument blocks: the host helpers of the launchers, and the two small
// kernels' bodies of the long-window paths (long_kernel.hip, faster_long_kernel.hip): the prepass that lists the long windows and the
// onHap pass over their reads.
#ifndef DD_KERNEL_COMMON_H
#define DD_KERNEL_COMMON_H
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>
#include "../../include/dindel_hmm.h"

/* Workspace of a long launch, the part both paths lay out alike: a 256-byte header, then i32 long_win[n_windows] (windows of class
 * DD_WIN_LONG with pairs, ascending), then at a 256-byte boundary i64 prefix[n_windows + 1] (prefix sums of their work), then the tiles.
 * Header words of one path alone (totals, rounds) are named in its own header. */
#define DD_LWS_HDR_COUNTER 0     /* u64 item counter */
#define DD_LWS_HDR_NWIN 8        /* i32 number of long windows */
#define DD_LWS_HDR_STATS 32      /* u64 stats[]: what a launch counts when the caller gives no words of its own */
#define DD_LWS_HEADER 256

namespace ddc {

static inline uint32_t up16(size_t v) { return (uint32_t)((v + 15u) & ~(size_t)15u); }

// The cap on dynamic LDS is a property of the function, not of a launch: it is raised ONCE per kernel (`done`: one word per kernel or
// template instance, bit d = done on device d) to the CU's 160 KiB, so that host threads launching the same kernel with different
// sizes cannot lower it under each other between the set and the launch.
inline hipError_t raise_lds_cap_once(const void *kernel, std::atomic<unsigned> &done)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned bit = 1u << (dev & 31);
    if (!(done.load(std::memory_order_acquire) & bit)) {
        e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        done.fetch_or(bit, std::memory_order_release);
    }
    return hipSuccess;
}

#ifdef __HIPCC__
// Prepass of a long launch, one workgroup of 1024 threads (sc, sp: 1024 words of LDS each), each thread over a contiguous segment of the
// windows [w_begin, w_end): lists the windows of class DD_WIN_LONG that have pairs, in order, with the prefix sums of weight(w) (at
// off_prefix); zeroes the item counter and the n_stats stats words.  Returns the sum of the weights to every thread.
template <class Args, class Weight>
__device__ __forceinline__ long long long_prepass(const Args &P, uint64_t off_prefix, int n_stats, int32_t *sc, long long *sp, Weight weight)
{
    const int t = threadIdx.x;
    const int n = P.w_end - P.w_begin;
    const int seg = (n + 1023) / 1024;
    const int lo = P.w_begin + t * seg, hi = min(lo + seg, P.w_end);
    auto is_long = [&](int w) { return P.win_class[w] == DD_WIN_LONG && P.win_pair_off[w + 1] - P.win_pair_off[w] > 0; };
    int cnt = 0;
    long long sum = 0;
    for (int w = lo; w < hi; w++)
        if (is_long(w)) { cnt++; sum += weight(w); }
    sc[t] = cnt; sp[t] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {         // inclusive scan (Hillis-Steele)
        const int c2 = t >= off ? sc[t - off] : 0;
        const long long p2 = t >= off ? sp[t - off] : 0;
        __syncthreads();
        sc[t] += c2; sp[t] += p2;
        __syncthreads();
    }
    int j = sc[t] - cnt;
    long long off = sp[t] - sum;
    int32_t *lwin = reinterpret_cast<int32_t *>(P.ws + DD_LWS_HEADER);
    int64_t *prefix = reinterpret_cast<int64_t *>(P.ws + off_prefix);
    for (int w = lo; w < hi; w++)
        if (is_long(w)) { lwin[j] = w; prefix[j] = off; j++; off += weight(w); }
    if (t == 1023) {
        prefix[sc[t]] = sp[t];
        *reinterpret_cast<unsigned long long *>(P.ws + DD_LWS_HDR_COUNTER) = 0ull;
        *reinterpret_cast<int32_t *>(P.ws + DD_LWS_HDR_NWIN) = sc[t];
        for (int i = 0; i < n_stats; i++) P.stats[i] = 0ull;
    }
    return sp[1023];
}

// onHap[r] of one read of a long window: 1 iff any haplotype of its window has a computed pair with !offHapHMQ (DInDel.cpp:1710, 1720).
// Runs after the long kernel, so that it sees that kernel's outputs; reads of windows outside [w_begin, w_end) or of another class are
// not touched — EVERY_CLASS (the wide launch, which has no main launch in front of it): reads of every class' windows are written.  (Both callers pass [read_begin, read_end) = the reads of the windows [w_begin, w_end), so the range test on w never
// decides anything; it only keeps a wrong caller from writing reads of a window the launch did not compute.)
template <bool EVERY_CLASS = false, class Args>
__device__ __forceinline__ void onhap_of_read(const Args &P)
{
    const int r = P.read_begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= P.read_end) return;
    int lo = 0, hi = P.n_windows;                      // window of read r: binary search in win_read_off
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (P.win_read_off[mid] <= r) lo = mid; else hi = mid;
    }
    const int w = lo;
    if (w < P.w_begin || w >= P.w_end || (!EVERY_CLASS && P.win_class[w] != DD_WIN_LONG)) return;
    const int H = P.win_hap_off[w + 1] - P.win_hap_off[w];
    const int r0 = P.win_read_off[w];
    const int R = P.win_read_off[w + 1] - r0;
    const int64_t base = P.win_pair_off[w] + (r - r0);
    int on = 0;
    for (int h = 0; h < H; h++) {
        const int64_t p = base + (int64_t)h * R;
        const int st = P.out.status[p];
        if (st != DD_PAIR_HAPSIZE && st != DD_PAIR_UNSUPPORTED && !P.out.offHapHMQ[p]) on = 1;
    }
    P.out.onHap[r] = (uint8_t)on;
}
#endif

} // namespace ddc
#endif
