// hapdist_kernel.hip — the block table of a window's empirical haplotype distribution: the end state of HaplotypeDistribution's
// constructor and insertRead (reference HaplotypeDistribution.cpp:29-45, 74-164, 343-436; HapBlock.cpp:20-70) inside the window's reference
// piece [rs, rs + L), computed in closed form instead of by inserting and splitting one segment at a time.
//
// Segments: the reference in pieces of 4 from rs; per read whose mate-unmapped bit (8) is clear and per operation, M and S lay their read
// letters from refPos on (S without advancing it), D is one position holding the byte '#' + min(len, 30), I goes to the insertion table,
// N and H show nothing; M / N advance refPos by len, D by min(len, 30).  A block boundary lies at every 4th position from rs, at every
// segment's first position and behind its last; a block's entries are the distinct strings its covering segments show, counted, in
// unsigned byte order, which a big-endian left-aligned u32 key reproduces because all entries of a block have its length.
// Insertion positions are created by their first I in (read, operation) order; every later non-I operation that is not its read's last
// and whose span [start, start of the next operation) holds the position adds one to the position's empty entry.
//
// Mapping: one wavefront per window, DD_HAPDIST_WAVES per workgroup, a persistent grid that draws windows from a counter (the draw of
// hapalign_kernel.hip).  Phase 1: lanes over reads walk their CIGARs, set cut bits in an LDS bitmap, look for what the reference throws
// on and count the window's insertion operations.  The set bits become the block starts (LDS).  Phase 2: lane = block, 64 blocks per pass;
// a wave-uniform walk over reads and operations (scalar state), each covering lane forms its key from the read's letters and keeps it in a
// sorted (key, count) list of DD_HAPDIST_MAX_DISTINCT registers pairs.  Phase 3 rides on the first pass's walk: lane = insertion position.
// A window with one pass and no insertion is walked once; any other is walked twice, first to learn whether it overflows and only then to
// store, so that a window whose status is not OK has nothing but its status written.
//
// Memory safety: every offset read from the batch is checked against the totals the offset arrays end with before it indexes anything
// (a read that fails makes the window DD_HAPDIST_HOST); a read's letters are indexed below its own base count only; stores go to
// blocks / entries / ins_ops / ins_pos below the window's capacity, which is checked against max_blk / max_ent / max_ins.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hapdist_kernel.h"

namespace dda {
namespace {

enum { OP_M = 0, OP_I = 1, OP_D = 2, OP_N = 3, OP_S = 4, OP_H = 5 };
enum { CUT_WORDS = DD_HAPDIST_MAX_WINDOW / 32 + 1, C = DD_HAPDIST_MAX_DISTINCT };
static_assert(CUT_WORDS <= 64, "one lane per bitmap word");

// LDS traffic of one wavefront is ordered; this keeps the compiler from moving it across the phases
#define DD_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

__device__ __forceinline__ int wave_sum(int v)
{
    #pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return __builtin_amdgcn_readfirstlane(v);
}

__device__ __forceinline__ int wave_or(int v)
{
    #pragma unroll
    for (int d = 32; d > 0; d >>= 1) v |= __shfl_xor(v, d);
    return __builtin_amdgcn_readfirstlane(v);
}

// inclusive prefix sum over the lanes
__device__ __forceinline__ int wave_scan(int v, int lane)
{
    #pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(v, d); if (lane >= d) v += o; }
    return v;
}

// one more observation of `key` in a lane's sorted list; the element carried along is the one being placed
__device__ __forceinline__ void list_add(uint32_t (&keys)[C], uint32_t (&cnts)[C], int &n, bool &ovf, uint32_t key, bool valid)
{
    uint32_t ck = key, cc = 1;
    #pragma unroll
    for (int i = 0; i < C; i++) {
        if (valid) {
            if (i < n) {
                if (keys[i] == ck) { cnts[i] += cc; valid = false; }
                else if (keys[i] > ck) { const uint32_t tk = keys[i], tc = cnts[i]; keys[i] = ck; cnts[i] = cc; ck = tk; cc = tc; }
            } else { keys[i] = ck; cnts[i] = cc; n = i + 1; valid = false; }
        }
    }
    if (valid) ovf = true;
}

__device__ __forceinline__ uint32_t key_of(const uint8_t *p, int blen)
{
    uint32_t k = (uint32_t)p[0] << 24;
    if (blen > 1) k |= (uint32_t)p[1] << 16;
    if (blen > 2) k |= (uint32_t)p[2] << 8;
    if (blen > 3) k |= (uint32_t)p[3];
    return k;
}

__device__ __forceinline__ int clamp30(long long a)
{
    return (int)(a < -(1ll << 30) ? -(1ll << 30) : a > (1ll << 30) ? (1ll << 30) : a);
}

} // namespace

__global__ void __launch_bounds__(64 * DD_HAPDIST_WAVES) dd_hapdist_kernel(HapdistArgs P)
{
    __shared__ uint32_t cutL[DD_HAPDIST_WAVES][CUT_WORDS];
    __shared__ uint16_t startL[DD_HAPDIST_WAVES][DD_HAPDIST_MAX_WINDOW + 2];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t *cut = cutL[wave];
    uint16_t *bst = startL[wave];
    const dd_hap_batch &B = P.b;
    const dd_hap_blocks &T = P.t;
    const uint8_t *ref_seq = reinterpret_cast<const uint8_t *>(B.ref_seq);
    const uint8_t *bases = reinterpret_cast<const uint8_t *>(B.bases);
    unsigned int *counter = P.hdr + DD_HAPDIST_HDR_COUNTER;
    const int n_windows = B.n_windows, n_reads = B.n_reads;
    // what the caller says its arrays hold: nothing is indexed at or past these
    const int tot_ref = B.win_ref_off[n_windows], tot_ops = B.read_op_off[n_reads], tot_bases = B.read_base_off[n_reads];

    unsigned int draws = 0;                                     // windows this wavefront drew: at most n_windows if the draw stays wave-uniform
    for (;;) {
        unsigned int drawn = atomicAdd(counter, lane == 0 ? 1u : 0u);          // every lane takes part in the draw (hapalign_kernel.hip)
        drawn = __builtin_amdgcn_readfirstlane(drawn);
        if (drawn >= (unsigned int)n_windows) break;
        if (++draws > (unsigned int)n_windows) {                // run-time guard of the draw (dd_hap_blocks_last_launch reports it)
            if (lane == 0) atomicAdd(P.hdr + DD_HAPDIST_HDR_TRIPS, 1u);
            break;
        }
        const int w = (int)drawn;
        const int rs = B.win_rs[w];
        const int ro = B.win_ref_off[w], L = B.win_ref_off[w + 1] - ro;
        const int r0 = B.win_read_off[w], r1 = B.win_read_off[w + 1];
        const long long bo = T.blk_off[w], bcap = (long long)T.blk_off[w + 1] - bo;
        const long long eo = T.ent_off[w], ecap = (long long)T.ent_off[w + 1] - eo;
        const long long io = T.ins_off[w], icap = (long long)T.ins_off[w + 1] - io;

        int status = DD_HAPDIST_OK;
        if (L > DD_HAPDIST_MAX_WINDOW) status = DD_HAPDIST_TOO_WIDE;
        else if (L <= 0 || rs < 0 || ro < 0 || ro + L > tot_ref || r0 < 0 || r1 < r0 || r1 > n_reads) status = DD_HAPDIST_HOST;
        else if (bo < 0 || bcap < 0 || bo + bcap > P.max_blk || eo < 0 || ecap < 0 || eo + ecap > P.max_ent || io < 0 || icap < 0 ||
                 io + icap > P.max_ins) status = DD_HAPDIST_OVERFLOW;

        int n_blocks = 0, nins_total = 0, left_all = 0;
        if (status == DD_HAPDIST_OK) {
            // ---- phase 1: cuts, what the reference throws on, the insertion operations inside the window
            if (lane < CUT_WORDS) cut[lane] = 0x11111111u;      // every 4th position from rs
            DD_WAVE_SYNC();
            int host = 0, nins = 0, left = 0;
            for (int r = r0 + lane; r < r1; r += 64) {
                if (B.read_flag[r] & 8) continue;               // BAM_FMUNMAP
                const int o0 = B.read_op_off[r], o1 = B.read_op_off[r + 1];
                const int b0 = B.read_base_off[r], nb = B.read_base_off[r + 1] - b0;
                if (o0 < 0 || o1 < o0 || o1 > tot_ops || o1 - o0 > 65535 || b0 < 0 || nb < 0 || nb > tot_bases - b0) { host = 1; continue; }
                long long refPos = B.read_pos[r];
                if (refPos < 0 && o1 > o0) { host = 1; continue; }
                long long lastPos = refPos, l = 0;
                int lastop = -1;
                for (int k = o0; k < o1; k++) {
                    const uint32_t c = B.ops[k];
                    const int op = (int)(c & 15u), len = (int)(c >> 4);
                    if (op == OP_M || op == OP_I || op == OP_S) { l += len; if (l > nb) { host = 1; break; } }
                    const int seglen = (op == OP_M || op == OP_S) ? len : (op == OP_D && len > 0) ? 1 : 0;
                    const long long a = refPos - rs;
                    if (seglen > 0) {
                        const long long e = a + seglen;         // the segment is [a, e)
                        if (a >= 0 && a <= L) atomicOr(&cut[a >> 5], 1u << (a & 31));
                        if (e >= 0 && e <= L) atomicOr(&cut[e >> 5], 1u << (e & 31));
                        if (a < 0) left |= e >= 0 ? 3 : 2;
                    }
                    if (op == OP_I && len > 0 && a >= 0 && a < L) nins++;
                    if (lastop != -1 && lastop != OP_I && lastPos == refPos && lastop != OP_S && lastop != OP_H) { host = 1; break; }   // "Mag niet."
                    lastPos = refPos;
                    if (op == OP_M || op == OP_N) refPos += len;
                    else if (op == OP_D) refPos += len > 30 ? 30 : len;
                    else if (op != OP_I && op != OP_S && op != OP_H) { host = 1; break; }       // "I don't know how to smoke this CIGAR"
                    lastop = op;
                }
            }
            if (wave_or(host)) status = DD_HAPDIST_HOST;
            nins_total = wave_sum(nins);
            left_all = wave_or(left);
            DD_WAVE_SYNC();

            // ---- block starts: the set bits below L, in order
            uint32_t m = 0;
            if (lane < CUT_WORDS) {
                m = cut[lane];
                const int lo = lane * 32;
                if (L <= lo) m = 0; else if (L - lo < 32) m &= (1u << (L - lo)) - 1u;
            }
            const int incl = wave_scan(__popc(m), lane);
            n_blocks = __builtin_amdgcn_readlane(incl, 63);
            int slot = incl - __popc(m);
            while (m) { const int j = __ffs(m) - 1; m &= m - 1; bst[slot++] = (uint16_t)(lane * 32 + j); }
            if (lane == 0) bst[n_blocks] = (uint16_t)L;         // n_blocks <= L <= DD_HAPDIST_MAX_WINDOW
            DD_WAVE_SYNC();
            if (status == DD_HAPDIST_OK && (n_blocks > bcap || nins_total > icap)) status = DD_HAPDIST_OVERFLOW;
        }

        int ent_total = 0, ins_n = 0, n_ins_pos = 0;
        int ins_p = -1, ins_cross = 0;                          // lane = insertion position, in order of creation
        if (status == DD_HAPDIST_OK) {
            const int passes = (n_blocks + 63) >> 6;
            const bool need_check = passes > 1 || nins_total > 0;
            bool ok = true;
            for (int sweep = need_check ? 0 : 1; sweep < 2 && ok; sweep++) {
                const bool writing = sweep == 1;
                ent_total = 0; ins_n = 0; n_ins_pos = 0; ins_p = -1; ins_cross = 0;
                bool ovf_ins = false;
                for (int pass = 0; pass < passes && ok; pass++) {
                    // ---- phase 2: lane = block
                    const int b = pass * 64 + lane;
                    const bool have = b < n_blocks;
                    const int bs = have ? (int)bst[b] : 0, be = have ? (int)bst[b + 1] : 0;
                    int blen = be - bs;
                    blen = blen < 1 ? 1 : blen > 4 ? 4 : blen;  // 1 ... 4 by the cuts at every 4th position
                    uint32_t keys[C], cnts[C];
                    #pragma unroll
                    for (int i = 0; i < C; i++) { keys[i] = 0; cnts[i] = 0; }
                    int n = 0;
                    bool ovf = false;
                    uint32_t refkey = 0;
                    if (have) { refkey = key_of(ref_seq + ro + bs, blen); keys[0] = refkey; cnts[0] = 1; n = 1; }     // bs + blen <= L

                    for (int r = r0; r < r1; r++) {             // wave-uniform walk
                        if (B.read_flag[r] & 8) continue;
                        const int o0 = B.read_op_off[r], o1 = B.read_op_off[r + 1];
                        const int b0 = B.read_base_off[r], nb = B.read_base_off[r + 1] - b0;
                        long long refPos = B.read_pos[r], l = 0;
                        for (int k = o0; k < o1; k++) {
                            const uint32_t c = B.ops[k];
                            const int op = (int)(c & 15u), len = (int)(c >> 4);
                            const long long a = refPos - rs;
                            const int a32 = clamp30(a);
                            bool cover = false;
                            uint32_t key = 0;
                            if ((op == OP_M || op == OP_S) && len > 0 && l + len <= nb) {
                                cover = have && a32 <= bs && bs + blen <= a32 + len;
                                if (cover) key = key_of(bases + b0 + (int)l + (bs - a32), blen);
                            } else if (op == OP_D && len > 0) {
                                cover = have && a32 == bs && blen == 1;
                                key = (uint32_t)('#' + (len > 30 ? 30 : len)) << 24;
                            }
                            if (op == OP_M || op == OP_I || op == OP_S) l += len;
                            const int adv = (op == OP_M || op == OP_N) ? len : op == OP_D ? (len > 30 ? 30 : len) : 0;
                            if (pass == 0) {
                                // ---- phase 3: lane = insertion position
                                if (op == OP_I) {
                                    if (len > 0 && a >= 0 && a < L) {
                                        const bool mine = lane < n_ins_pos && ins_p == a32;
                                        if (!__any(mine)) {
                                            if (n_ins_pos >= DD_HAPDIST_MAX_INS_POS) ovf_ins = true;
                                            else { if (lane == n_ins_pos) { ins_p = a32; ins_cross = 0; } n_ins_pos++; }
                                        }
                                        if (writing && lane == 0 && ins_n < icap) {
                                            T.ins_ops[(io + ins_n) * 2] = (uint32_t)(r - r0);
                                            T.ins_ops[(io + ins_n) * 2 + 1] = ((uint32_t)(k - o0) << 16) | (uint32_t)a32;
                                        }
                                        ins_n++;
                                    }
                                } else if (k < o1 - 1 && adv > 0) {
                                    if (lane < n_ins_pos && a32 <= ins_p && ins_p < a32 + adv) ins_cross++;
                                }
                            }
                            list_add(keys, cnts, n, ovf, key, cover);
                            refPos += adv;
                        }
                    }

                    const int incl = wave_scan(have ? n : 0, lane);
                    const int total = __builtin_amdgcn_readlane(incl, 63);
                    if (__any(ovf) || ovf_ins || ent_total + total > ecap || ins_n > icap) ok = false;
                    if (ok && writing && have) {
                        int ref_idx = 0;
                        #pragma unroll
                        for (int i = 0; i < C; i++) if (i < n && keys[i] == refkey) ref_idx = i;
                        T.blocks[bo + b] = (uint32_t)bs | ((uint32_t)blen << 16) | ((uint32_t)n << 20) | ((uint32_t)ref_idx << 26);
                        uint32_t *e = T.entries + (eo + ent_total + (incl - n)) * 2;
                        #pragma unroll
                        for (int i = 0; i < C; i++) if (i < n) { e[2 * i] = keys[i]; e[2 * i + 1] = cnts[i]; }
                    }
                    ent_total += total;
                }
            }
            if (!ok) status = DD_HAPDIST_OVERFLOW;
        }

        if (status == DD_HAPDIST_OK) {
            if (lane < n_ins_pos) { T.ins_pos[(io + lane) * 2] = (uint32_t)ins_p; T.ins_pos[(io + lane) * 2 + 1] = (uint32_t)ins_cross; }
            if (lane == 0) {
                T.n_blocks[w] = n_blocks; T.n_entries[w] = ent_total; T.n_ins_ops[w] = ins_n; T.n_ins_pos[w] = n_ins_pos; T.left[w] = left_all;
            }
        }
        if (lane == 0) T.status[w] = status;
    }
    if (lane == 0) atomicMax(P.hdr + DD_HAPDIST_HDR_MAX_DRAWS, draws);
}

hipError_t launch_hapdist(const HapdistArgs &A, hipStream_t st)
{
    if (A.b.n_windows <= 0) return hipSuccess;
    return zero_and_launch(dd_hapdist_kernel, persistent_grid(A.b.n_windows, DD_HAPDIST_WAVES, DD_HAPDIST_MAX_BLOCKS), 64 * DD_HAPDIST_WAVES, 0,
                           A.hdr, DD_HAPDIST_WS_BYTES, st, A);
}

} // namespace dda
