// indel_keys_kernel.hip — the --faster model's indel-map key count on the device: per (haplotype, read) pair the number of distinct keys
// its record's indel map would hold, from the hpos the likelihood kernels left in HBM, so that the window loop needs 2 bytes per pair
// instead of the pair's whole per-base alignment.  indel_keys_kernel.h is the definition (ik_classify), shared with the CPU evaluation.
//
// One wavefront per pair, 64 read bases at a time, a persistent grid striding over the pairs (cigar_kernel.hip's mapping); no counter and
// no atomics.  A lane classifies the step INTO its base with ik_classify; its left neighbour comes from a cross-lane read, lane 0's from
// the chunk before (carry).  lhp of a run that starts with the bare code is one past the nearest earlier entry with a position: one ballot
// and one cross-lane read, carried across chunks likewise.  The few events of a chunk are replayed one by one on wave-uniform state into
// the list of distinct keys, which lives in one register: lane i holds key i, membership is one ballot.  Every loop is bounded by L
// (chunks) or by 64 (a chunk's events).  Lanes beyond the read load nothing.  No floating point; lane 0 stores the result with an
// ordinary vector store.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "indel_keys_kernel.h"

namespace ddi {
namespace {

__device__ __forceinline__ uint64_t bits_below(int n) { return n >= 64 ? ~0ull : ((1ull << n) - 1ull); }

// the count of `pair` (wave-uniform); every lane of the wavefront calls it with the same arguments
__device__ __forceinline__ int count_keys(const IndelKeysArgs &P, const int64_t pair, const int lane)
{
    int lo = 0, hi = P.n_windows;                                  // window of this pair: binary search in the pair offsets
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (P.win_pair_off[mid] <= pair) lo = mid; else hi = mid;
    }
    const int w = lo;
    const int q0 = P.win_read_off[w], R = P.win_read_off[w + 1] - q0;
    const int idx = (int)(pair - P.win_pair_off[w]);
    const int h = idx / R, r = idx - h * R;
    const int q = q0 + r;
    const int rs0 = P.read_seq_off[q0], SL = P.read_seq_off[q0 + R] - rs0;
    const int rb = P.read_seq_off[q], L = P.read_seq_off[q + 1] - rb;
    const int16_t *hp = P.hpos + P.win_hpos_off[w] + (int64_t)h * SL + (rb - rs0);

    int my_key = 0, nk = 0;                                        // the distinct keys: lane i holds key i, i < nk
    int carry = DD_HPOS_LO;                                        // the entry in front of this chunk
    int carry_lhp = 1;                                             // lhp in front of this chunk
    for (int c0 = 0; c0 < L; c0 += 64) {
        const int b = c0 + lane;
        const int cur = b < L ? (int)hp[b] : DD_HPOS_LO;           // beyond the read: neither inserted nor a position, never an event
        int prev = __shfl_up(cur, 1);
        if (lane == 0) prev = carry;
        const uint64_t pos = __ballot(cur >= 0);
        const uint64_t before = pos & bits_below(lane);
        int lhp = __shfl(cur, before ? 63 - __builtin_clzll(before) : 0) + 1;
        if (!before) lhp = carry_lhp;
        int key = 0;
        const int cls = b < L ? ik_classify(prev, cur, &key) : IK_NONE;
        if (cls == IK_RUN_BARE) key = lhp;
        uint64_t ev = __ballot(cls != IK_NONE);
        while (ev) {                                               // at most 64 events in a chunk
            const int e = __builtin_ctzll(ev);
            const int k = __builtin_amdgcn_readlane(key, e);
            if (!__ballot(lane < nk && my_key == k)) {
                if (nk == DD_INDEL_KEYS_CAP) return DD_INDEL_KEYS_OVERFLOW;
                if (lane == nk) my_key = k;
                nk++;
            }
            ev &= ev - 1;
        }
        carry = __builtin_amdgcn_readlane(cur, 63);
        if (pos) carry_lhp = __builtin_amdgcn_readlane(cur, 63 - __builtin_clzll(pos)) + 1;
    }
    return nk;
}

} // namespace

__global__ void __launch_bounds__(64 * DD_INDEL_KEYS_WAVES) dd_indel_keys_kernel(IndelKeysArgs P)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t stride = (int64_t)gridDim.x * DD_INDEL_KEYS_WAVES;
    const int64_t pair_end = P.pair_end >= 0 ? P.pair_end : P.win_pair_off[P.n_windows];
    for (int64_t pair = P.pair_begin + (int64_t)blockIdx.x * DD_INDEL_KEYS_WAVES + wave; pair < pair_end; pair += stride) {
        int v = DD_INDEL_KEYS_NOT_COMPUTED;                        // no alignment was computed: marked, hpos not read
        if (!P.pair_status || P.pair_status[pair] == DD_PAIR_OK) v = count_keys(P, pair, lane);
        if (lane == 0) P.out[pair] = (int16_t)v;
    }
}

hipError_t launch_indel_keys(const IndelKeysArgs &A, hipStream_t st)
{
    const int64_t n = A.max_pairs;
    if (n <= 0) return hipSuccess;
    int64_t blocks = (n + DD_INDEL_KEYS_WAVES - 1) / DD_INDEL_KEYS_WAVES;
    if (blocks > DD_INDEL_KEYS_MAX_BLOCKS) blocks = DD_INDEL_KEYS_MAX_BLOCKS;
    hipLaunchKernelGGL(dd_indel_keys_kernel, dim3((unsigned)blocks), dim3(64 * DD_INDEL_KEYS_WAVES), 0, st, A);
    return hipGetLastError();
}

} // namespace ddi
