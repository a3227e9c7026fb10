// realign_kernel.hip — the realigned reads on the device: which haplotype each read is realigned to, and the CIGAR of that pair alone.
//
// The specification is host/realigned_bam.cpp (reference DInDel.cpp:498-520 for the pooled rule, :596-611 for the diploid rule):
//     FIRST_MAX   a read that is on no haplotype (onHap == 0) chooses nothing; otherwise the first haplotype whose ll is strictly greater
//                 than the running maximum, which starts at -inf; haplotype 0 when none compares greater
//     PAIR        of the window's pair (h1, h2): within 1e-8 the one with fewer indels (h2 on equal counts), otherwise the likelier one
//                 (h2 unless ll[h1] > ll[h2])
// Both are fp64 subtract / compare / select in the host's order, so the choice is the host's bit for bit: NaN never compares greater (or
// below 1e-8), which is what the host's `>` and `<` do.  No max instruction is used.
//
// One wavefront takes 64 consecutive reads of the batch, one per lane.  A lane finds its read's window by binary search in win_read_off
// (the last window whose offset is <= q: of several windows that share an offset only the last one holds reads), then runs over the
// window's haplotypes serially: ll[h * R + r] is contiguous over the lanes of one window, 512 bytes per step when the window fills the
// wavefront.  The chosen pairs are then walked one after the other by the whole wavefront (cigar_walk.h, the walk of cigar_kernel.hip, 64
// read bases per step), each with wave-uniform arguments taken from its lane, and written at the READ's index.  A read for which nothing
// is chosen is finished by its own lane.  Persistent grid: the wavefronts stride over the 64-read items.
//
// No LDS, no floating point beyond the compares; ordinary vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "realign_kernel.h"
#include "cigar_walk.h"

namespace ddc {

__global__ void __launch_bounds__(64 * DD_CIGAR_WAVES) dd_realign_kernel(RealignArgs P)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t stride = (int64_t)gridDim.x * DD_CIGAR_WAVES * 64;
    const CigarArgs &C = P.cig;
    for (int64_t q_base = P.read_begin + ((int64_t)blockIdx.x * DD_CIGAR_WAVES + wave) * 64; q_base < P.read_end; q_base += stride) {
        const int64_t q = q_base + lane;
        int64_t pair = -1;                                             // the chosen pair; -1: nothing to walk for this lane
        if (q < P.read_end) {
            int lo = 0, hi = C.n_windows;                              // window of this read: the last one that starts at or in front of it
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (C.win_read_off[mid] <= q) lo = mid; else hi = mid;
            }
            const int w = lo;
            const int q0 = C.win_read_off[w], R = C.win_read_off[w + 1] - q0, r = (int)(q - q0);
            const int g0 = C.win_hap_off[w], H = C.win_hap_off[w + 1] - g0;
            const double *ll = P.ll + C.win_pair_off[w] + r;           // ll[h * R]: haplotype h with this read
            int hidx = -1, none = DD_REALIGN_NO_HAPS;
            if (H > 0 && P.mode == DD_REALIGN_FIRST_MAX) {
                if (P.on_hap && !P.on_hap[q]) {
                    none = DD_REALIGN_OFF_HAP;
                } else {
                    double best = -__builtin_huge_val();
                    hidx = 0;
                    for (int h = 0; h < H; h++) {
                        const double v = ll[(int64_t)h * R];
                        if (v > best) { best = v; hidx = h; }
                    }
                }
            } else if (H > 0) {
                const int h1 = P.win_hap_pair[2 * w], h2 = P.win_hap_pair[2 * w + 1];
                if (h1 < 0 || h1 >= H || h2 < 0 || h2 >= H) {
                    none = DD_REALIGN_BAD_PAIR;
                } else {
                    const double l1 = ll[(int64_t)h1 * R], l2 = ll[(int64_t)h2 * R];
                    if (__builtin_fabs(l1 - l2) < 1e-8) hidx = P.hap_n_indels[g0 + h1] < P.hap_n_indels[g0 + h2] ? h1 : h2;
                    else hidx = l1 > l2 ? h1 : h2;
                }
            }
            P.hap[q] = hidx;
            if (hidx >= 0) {
                pair = C.win_pair_off[w] + (int64_t)hidx * R + r;
            } else {
                C.out.status[q] = none; C.out.n_ops[q] = 0; C.out.ref_off[q] = -1;
            }
        }
        // the chosen pairs of this item, one after the other on the whole wavefront
        for (uint64_t todo = __ballot(pair >= 0); todo; todo &= todo - 1) {
            const int j = __builtin_ctzll(todo);
            const uint32_t p_lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)pair, j);
            const uint32_t p_hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)pair >> 32), j);
            cigar_walk(C, (int64_t)(((uint64_t)p_hi << 32) | p_lo), C.out, q_base + j, lane);
        }
    }
}

hipError_t launch_realign(const RealignArgs &A, hipStream_t st)
{
    const int64_t n = (int64_t)A.read_end - A.read_begin;
    if (n <= 0) return hipSuccess;
    int64_t blocks = (n + 64 * DD_CIGAR_WAVES - 1) / (64 * DD_CIGAR_WAVES);
    if (blocks > DD_CIGAR_MAX_BLOCKS) blocks = DD_CIGAR_MAX_BLOCKS;
    hipLaunchKernelGGL(dd_realign_kernel, dim3((unsigned)blocks), dim3(64 * DD_CIGAR_WAVES), 0, st, A);
    return hipGetLastError();
}

} // namespace ddc
