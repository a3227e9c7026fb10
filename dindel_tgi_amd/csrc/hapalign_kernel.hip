// hapalign_kernel.hip — global affine-gap alignment of candidate haplotypes against their window's reference sequence: the arithmetic of
// DetInDel::alignHaplotypes (reference DInDel.cpp:1427-1524), which calls SeqAn's globalAlignment with Score<int>(-1, -460, -100, -960)
// and no free end gaps.  The specification is the Gotoh code that call selects (seqan/graph_align/graph_align_gotoh.h: _align_gotoh,
// _align_gotoh_trace), reproduced with its strict comparisons and its traceback state machine, because its tie rules decide where an
// indel inside a repeat lands.
//
// Columns are the reference window (str1), rows the haplotype (str2).  Both are read as seqan::Dna: A/a 0, C/c 1, G/g 2, T/t/U/u 3 and
// every other byte 0.  Per cell, in this order:
//     vert = max(mat[row-1, col] - 960, vert - 100)              open bit (8) set only when the first is greater
//     hor  = max(mat[row, col-1] - 960, hor[row] - 100)          open bit (4), same rule
//     mat  = diag + (-1 | -460); vert if vert > mat (2); then hor if hor > mat (1)
// All of it int32.
//
// Mapping: one wavefront per pair, DD_ALIGN_WAVES per workgroup, a persistent grid that draws pairs from a counter in the workspace header.
// Lane l owns the K = ceil(len2 / 64) rows l K + 1 ... l K + K; at step t it works on column t - l + 1 and receives mat and vert of the row
// above its block from lane l - 1 (computed one step earlier) with a wave shift, and the column's reference base the same way.  The lane's
// mat and hor columns and its rows' base codes live in LDS as [k][lane] (conflict-free: consecutive lanes on consecutive banks).  One byte
// of trace per cell goes to the wavefront's tile in the workspace, stored by step so that a step's stores are contiguous.  The tile is
// then walked backwards, serially (every lane runs the walk on wave-uniform state, lane 0 stores): every haplotype base gets the
// reference offset it is paired with, or -1 - (reference bases left of its column) when it faces a gap (dd_align_result).
//
// Memory safety: a pair is computed only when 1 <= len1 <= max_ref_len and 1 <= len2 <= max_hap_len, the lengths the tile and the LDS rows
// are sized for; lanes beyond len2 load and store nothing; the traceback's cursors are clamped at 0.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include "hapalign_kernel.h"

namespace dda {
namespace {

enum { TV_DIAG = 0, TV_HOR = 1, TV_VERT = 2, BIT_HOR_OPEN = 4, BIT_VERT_OPEN = 8 };
enum { S_MATCH = -1, S_MISMATCH = -460, S_GAP_EXTEND = -100, S_GAP_OPEN = -960 };

// seqan::Dna of a byte
__device__ __forceinline__ int dna_code(unsigned b)
{
    b &= 0xDFu;                     // lower case onto upper case; no other byte lands on a letter
    return b == 'C' ? 1 : b == 'G' ? 2 : (b == 'T' || b == 'U') ? 3 : 0;
}

// mat of the DP's first row or first column at distance n >= 0 from the corner
__device__ __forceinline__ int edge_mat(int n) { return n == 0 ? 0 : S_GAP_OPEN + S_GAP_EXTEND * (n - 1); }

// The alignment, written from its end: (tv, n) segments as _align_gotoh_trace hands them to _align_trace_print.  i / j: reference and
// haplotype bases not yet emitted; a base that faces a gap records i, which places its column among deleted reference bases (SeqAn puts
// a deletion in front of an insertion that touches it, except where the traceback's edge remainder says otherwise).  Every lane runs the walk (the state is wave-uniform); only the writer lane stores.
struct Emitter {
    int16_t *out;
    int i, j;
    bool writer;
    __device__ __forceinline__ void put(int tv, int n)
    {
        if (tv == TV_DIAG) { for (; n > 0 && i > 0 && j > 0; n--) { --j; --i; if (writer) out[j] = (int16_t)i; } }
        else if (tv == TV_HOR) { i = n < i ? i - n : 0; }
        else { for (; n > 0 && j > 0; n--) { --j; if (writer) out[j] = (int16_t)(-1 - i); } }      // DD_ALIGN_GAP: the reference bases left of the column
    }
};

} // namespace

__global__ void __launch_bounds__(64 * DD_ALIGN_WAVES) dd_hapalign_kernel(AlignArgs P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lds_rows = 64 * P.K;
    int32_t *matL = reinterpret_cast<int32_t *>(lds_raw) + (size_t)wave * 2 * lds_rows;
    int32_t *horL = matL + lds_rows;
    uint8_t *hapL = lds_raw + (size_t)DD_ALIGN_WAVES * 8 * lds_rows + (size_t)wave * lds_rows;
    unsigned char *tile = P.ws + DD_ALIGN_WS_HEADER + ((size_t)blockIdx.x * DD_ALIGN_WAVES + wave) * P.tile_bytes;
    unsigned int *counter = reinterpret_cast<unsigned int *>(P.ws);

    unsigned int draws = 0;                                     // pairs this wavefront drew: at most n_pairs if the draw stays wave-uniform
    for (;;) {
        // Every lane takes part in the draw (lane 0 adds one, the others nothing) and the wavefront continues with lane 0's value.  Written
        // as `if (lane == 0) drawn = atomicAdd(...)`, the compiler threaded the back edges that come from code behind another lane test
        // past the draw for lanes 1 ... 63, which then looped without lane 0 on a pair number nobody had drawn.
        unsigned int drawn = atomicAdd(counter, lane == 0 ? 1u : 0u);
        drawn = __builtin_amdgcn_readfirstlane(drawn);
        if (drawn >= (unsigned int)P.n_pairs) break;
        if (++draws > (unsigned int)P.n_pairs) {                // run-time guard of the draw (dd_align_last_launch reports it): never true while
            if (lane == 0) atomicAdd(counter + DD_ALIGN_HDR_TRIPS, 1u);   // every draw comes from the counter
            break;
        }
        const int pair = (int)drawn;

        const int h0 = P.hap_off[pair];
        const int len2 = P.hap_off[pair + 1] - h0;
        const int r = P.pair_ref[pair];
        const bool ref_ok = r >= 0 && r < P.n_refs;
        const int r0 = ref_ok ? P.ref_off[r] : 0;
        const int len1 = ref_ok ? P.ref_off[r + 1] - r0 : 0;
        int16_t *out = P.ref_pos + h0;
        int status = DD_ALIGN_OK;
        if (!ref_ok) status = DD_ALIGN_BAD_REF;
        else if (len1 <= 0 || len2 <= 0) status = DD_ALIGN_EMPTY;
        else if (len1 > P.max_ref_len || len2 > P.max_hap_len) status = DD_ALIGN_TOO_LONG;
        if (status != DD_ALIGN_OK) {
            for (int b = lane; b < len2; b += 64) out[b] = -1;
            if (lane == 0) { P.score[pair] = 0; P.status[pair] = status; }
            continue;
        }

        const int K = (len2 + 63) >> 6;                         // rows per lane for this pair (<= P.K)
        const int n_lanes = (len2 + K - 1) / K;                 // lanes that own a row
        const int row_base = lane * K;                          // 0-based index of the lane's first row
        int my_rows = len2 - row_base;
        my_rows = my_rows < 0 ? 0 : my_rows > K ? K : my_rows;
        for (int k = 0; k < my_rows; k++) {                     // first column (:196-199) and the rows' bases
            const int m = edge_mat(row_base + k + 1);
            matL[k * 64 + lane] = m;
            horL[k * 64 + lane] = m + S_GAP_OPEN - S_GAP_EXTEND;
            hapL[k * 64 + lane] = (uint8_t)dna_code(P.hap_seq[h0 + row_base + k]);
        }

        int above_prev = edge_mat(row_base);                    // mat[row above the block, previous column]: the block's first diagonal
        int out_mat = 0, out_vert = 0;                          // mat and vert of the block's last row in the column just done
        int ref_chunk = 0, ref_base = 0;
        const int steps = len1 + n_lanes - 1;
        for (int t = 0; t < steps; t++) {
            if ((t & 63) == 0) ref_chunk = t + lane < len1 ? dna_code(P.ref_seq[r0 + t + lane]) : 0;
            const int entering = __shfl(ref_chunk, t & 63);     // base of column t + 1, which lane 0 starts now
            int rb = __shfl_up(ref_base, 1);
            int above = __shfl_up(out_mat, 1), vert = __shfl_up(out_vert, 1);
            const int col = t - lane + 1;
            if (lane == 0) {                                    // first row (:206-207)
                rb = entering;
                above = edge_mat(col);
                vert = above + S_GAP_OPEN - S_GAP_EXTEND;
            }
            ref_base = rb;
            if (col >= 1 && col <= len1 && my_rows > 0) {
                int diag = above_prev;
                above_prev = above;
                int up = above;
                unsigned char *tp = tile + (size_t)t * (size_t)len2 + row_base;
                for (int k = 0; k < K; k++) {                   // wave-uniform trip count; a lane's rows end at my_rows
                    if (k >= my_rows) break;
                    int bits = 0;
                    int a = up + S_GAP_OPEN, b = vert + S_GAP_EXTEND;
                    if (a > b) { vert = a; bits = BIT_VERT_OPEN; } else vert = b;
                    const int left = matL[k * 64 + lane];
                    a = left + S_GAP_OPEN; b = horL[k * 64 + lane] + S_GAP_EXTEND;
                    int hor;
                    if (a > b) { hor = a; bits |= BIT_HOR_OPEN; } else hor = b;
                    int best = diag + ((int)hapL[k * 64 + lane] == rb ? S_MATCH : S_MISMATCH), tv = TV_DIAG;
                    if (vert > best) { best = vert; tv = TV_VERT; }
                    if (hor > best) { best = hor; tv = TV_HOR; }
                    diag = left;
                    matL[k * 64 + lane] = best;
                    horL[k * 64 + lane] = hor;
                    tp[k] = (unsigned char)(bits | tv);
                    up = best;
                }
                out_mat = up;
                out_vert = vert;
            }
        }

        // bottom right corner (:256-260): the lane that owns the last row finished the last column in the last step
        const int last_lane = (len2 - 1) / K, last_k = (len2 - 1) - last_lane * K;
        int fin_mat = 0, fin_dir = TV_DIAG;
        if (lane == last_lane) {
            fin_mat = matL[last_k * 64 + lane];
            if (horL[last_k * 64 + lane] == fin_mat) fin_dir = TV_HOR;
            else if (out_vert == fin_mat) fin_dir = TV_VERT;
        }
        fin_mat = __shfl(fin_mat, last_lane);
        fin_dir = __shfl(fin_dir, last_lane);
        __threadfence();                                        // the tile was written by all lanes and is read by lane 0

        // _align_gotoh_trace (:33-136), serial.  The walk's state is the same in every lane and every lane runs it, so that the wavefront
        // stays together up to the next draw: with the walk inside `if (lane == 0)` the compiler let the other 63 lanes run ahead into
        // the next iteration, where readfirstlane then read a lane that had drawn nothing.  Lane 0 alone stores.
        {
            if (lane == 0) { P.score[pair] = fin_mat; P.status[pair] = DD_ALIGN_OK; }
            Emitter em = {out, len1, len2, lane == 0};
            int l1 = len1, l2 = len2;
            #define DD_TRACE_CELL(c, rw) ((int)tile[(size_t)((c) - 1 + ((rw) - 1) / K) * (size_t)len2 + ((rw) - 1)])
            int ntv = DD_TRACE_CELL(l1, l2);
            int tv = TV_DIAG;
            if (fin_dir == TV_DIAG) tv = ntv & 3;
            else if (fin_dir == TV_HOR) {
                if (ntv & BIT_HOR_OPEN) { em.put(TV_HOR, 1); --l1; } else tv = TV_HOR;
            } else {
                if (ntv & BIT_VERT_OPEN) { em.put(TV_VERT, 1); --l2; } else tv = TV_VERT;
            }
            int seg = 0, tv_old = tv;
            while (l1 != 0 && l2 != 0) {                        // the source's do-while would index the trace at -1 after an opening first step at the edge
                ntv = DD_TRACE_CELL(l1, l2);
                if (tv == TV_DIAG) tv = ntv & 3;
                else if (tv == TV_HOR) tv = (ntv & BIT_HOR_OPEN) ? TV_DIAG : TV_HOR;
                else tv = (ntv & BIT_VERT_OPEN) ? TV_DIAG : TV_VERT;
                if (tv == TV_DIAG) {
                    if (tv != tv_old) {
                        if (tv_old == TV_VERT) --l2; else --l1;
                        em.put(tv_old, ++seg);
                        tv_old = tv; seg = 0;
                    } else { ++seg; --l1; --l2; }
                } else if (tv == TV_HOR) {
                    if (tv != tv_old) {
                        em.put(tv_old, seg);
                        if (ntv & BIT_HOR_OPEN) { em.put(TV_HOR, 1); --l1; tv = TV_DIAG; seg = 0; }
                        else { tv_old = tv; seg = 1; --l1; }
                    } else { ++seg; --l1; }
                } else {
                    if (tv != tv_old) {
                        em.put(tv_old, seg);
                        if (ntv & BIT_VERT_OPEN) { em.put(TV_VERT, 1); --l2; tv = TV_DIAG; seg = 0; }
                        else { tv_old = tv; seg = 1; --l2; }
                    } else { ++seg; --l2; }
                }
            }
            #undef DD_TRACE_CELL
            if (seg) em.put(tv_old, seg);
            if (l1 != 0) em.put(TV_HOR, l1);                    // the sequence remainder at the matrix edge
            else if (l2 != 0) em.put(TV_VERT, l2);
            em.put(TV_VERT, em.j);                              // nothing is left here when the segments add up; never leave a base unwritten
        }
    }
    if (lane == 0) atomicMax(counter + DD_ALIGN_HDR_MAX_DRAWS, draws);
}

hipError_t launch_hapalign(const AlignArgs &A, unsigned grid, hipStream_t st)
{
    if (A.n_pairs <= 0) return hipSuccess;
    const size_t lds = align_lds_bytes(A.K);
    // the dynamic-LDS ceiling of the kernel is raised once per device, to the most any launch asks for: the value never changes afterwards,
    // so host threads that launch batches of different K side by side do not race on it
    static std::atomic<unsigned long long> raised(0ull);
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(raised.load() & bit)) {
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(dd_hapalign_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)align_lds_bytes((DD_LONG_MAX_HAP_LEN + 63) / 64));
        if (e != hipSuccess) return e;
        raised.fetch_or(bit);
    }
    return zero_and_launch(dd_hapalign_kernel, grid, 64 * DD_ALIGN_WAVES, lds, A.ws, DD_ALIGN_WS_HEADER, st, A);
}

} // namespace dda
