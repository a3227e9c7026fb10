// faster_long_kernel.hip — the "--faster" model (ObservationModelS) for the windows faster_kernel.hip skips:
// haplotypes of 767..4,094 bp, reads of 1,025..4,096 bp (opt-in: DD_OPT_LONG_WINDOWS_FASTER).
//
// Per (haplotype, read) pair it computes exactly what dd_faster_kernel computes (see that file's header for the model and the reference
// lines): HapHash 4-mer voting for <= 15 candidate diagonals, the Viterbi over S <= 16 relative-position states x {not inserted,
// inserted} from both read ends to bMid, mapState, hpos, firstBase / lastBase, the coverage flags.  Same fp64 terms in the same order,
// the same order in which candidates meet `nv > cur + 1e-7`, tables from dd_build_tables, -ffp-contract=off.  Quirks kept: the last 4-mer
// of the haplotype is never hashed, non-ACGT hashes as 'A', offHap / offHapHMQ always 0, states right of the haplotype map to hap base
// hlen-1.  The model itself is shared with that kernel: helpers in faster_model.h, SStateHMM in faster_sstate.inc, the end of a pair in
// faster_pair_end.inc; the prepass and the onHap pass are shared with long_kernel.hip (kernel_common.h).
//
// Why a kernel of its own: dd_faster_kernel keeps a pair's vote histogram (2 B per diagonal), read (2 B per base) and back-pointers
// (16 B per base) in LDS — ~89 KB per pair at 4,094 x 4,096, and a wavefront needs two such areas.  Here
//   LDS  (block-shared)  the haplotype bytes, its 4-mer bucket index (uint16 positions: hlen <= 4,094), the quality table;
//        (per pair)      the read (u16 per base), a 512-byte scratch X (the per-base exchange slots; later the 16-row staging buffer of the
//                        backtrack, then the coverage bitmap), the sorted relative positions;
//   HBM  (per 16-lane group, one tile of the workspace)  back-pointers bt[L][16] (a row is one 16-byte segment, written as the row is
//        computed, read back 16 rows per load with the next load in flight), and the vote histogram, whose bytes hold the state path
//        once the diagonals are chosen (read and written 16 rows = 32 B at a time).
// 16-bit vote bins cannot overflow: bin (diagonal) i receives a vote from read 4-mer x only through haplotype position i + x - L, which
// the bucket index lists once, so a bin gets at most one vote per read 4-mer: <= L - 3 <= 4,093.  The selection key packs
// (votes << 16) | (0xFFFF - bin): bin <= hlen + L <= 8,190.  The 15 winners are taken in descending key order (keys are distinct), each
// round looking only at keys below the previous winner, so the histogram is never modified after the voting.
//
// Mapping: one workgroup (4 wavefronts) works on ONE haplotype at a time — 16 pairs, 16 lanes each, lane d owns diagonal d as in
// dd_faster_kernel.  Persistent grid: an item is (haplotype of a long window, up to 16 x rounds consecutive reads); workgroups draw items
// from the counter in the workspace header (this workspace's own, not the main path's) and rebuild the haplotype index only when the
// haplotype changes.
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>
#include "hmm_kernel.h"
#include "kernel_common.h"
#include "faster_long_kernel.h"
#include "faster_model.h"

namespace ddf {

using namespace ddfm;
using ddc::up16;

// HBM tile traffic between lanes of one wavefront: the stores have to have left the wave before another lane loads them
__device__ __forceinline__ void tile_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// One workgroup: the windows of class DD_WIN_LONG with pairs, how many reads an item takes, and the items' prefix sums.
__global__ void __launch_bounds__(1024) dd_faster_long_prepass(const FLArgs P)
{
    __shared__ int32_t sc[1024];
    __shared__ long long sp[1024];
    const int t = threadIdx.x;
    const int n = P.w_end - P.w_begin;
    const int seg = (n + 1023) / 1024;
    const int lo = P.w_begin + t * seg, hi = min(lo + seg, P.w_end);
    // pairs of the long windows -> reads per item
    long long pairs = 0;
    for (int w = lo; w < hi; w++) {
        const long long np = P.win_pair_off[w + 1] - P.win_pair_off[w];
        if (P.win_class[w] == DD_WIN_LONG && np > 0) pairs += np;
    }
    sp[t] = pairs;
    __syncthreads();
    for (int off = 512; off >= 1; off >>= 1) {
        if (t < off) sp[t] += sp[t + off];
        __syncthreads();
    }
    const long long total_pairs = sp[0];
    __syncthreads();
    long long rounds = total_pairs / ((long long)DD_FL_PAIRS * 4 * (P.grid > 0 ? P.grid : 1));   // >= 4 items per workgroup when there is that much work
    rounds = rounds < 1 ? 1 : (rounds > DD_FL_MAX_ROUNDS ? DD_FL_MAX_ROUNDS : rounds);
    const int per_item = (int)rounds * DD_FL_PAIRS;
    // items per window = haplotypes x ceil(reads / per_item)
    const long long items = ddc::long_prepass(P, P.off_ioff, 4, sc, sp, [&](int w) {
        const int H = P.win_hap_off[w + 1] - P.win_hap_off[w], R = P.win_read_off[w + 1] - P.win_read_off[w];
        return (long long)H * ((R + per_item - 1) / per_item);
    });
    if (t == 1023) {
        *reinterpret_cast<int32_t *>(P.ws + DD_FL_HDR_ROUNDS) = (int32_t)rounds;
        *reinterpret_cast<int64_t *>(P.ws + DD_FL_HDR_ITEMS) = items;
        *reinterpret_cast<int64_t *>(P.ws + DD_FL_HDR_PAIRS) = total_pairs;
    }
}

// 2 waves per SIMD at most, as dd_faster_kernel: the 16-source loops want ~200 VGPRs.  Resident workgroups per CU are LDS-limited (plan.cpp).
__global__ void __launch_bounds__(DD_FL_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) dd_faster_long_kernel(const FLArgs P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, l16 = lane & 15, grp = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const double *T = P.tables;
    const double l1mE = T[TC_FAST + 0], lE = T[TC_FAST + 1], NIf = T[TC_FAST + 2], hqOn = T[TC_FAST + 3], hqOff = T[TC_FAST + 4];
    const double IIf = -0.25;
    // block-shared
    double2 *qt = reinterpret_cast<double2 *>(smem + P.lds_off_qt);          // {log match, log mismatch} per quality index
    unsigned char *shHap = smem + P.lds_off_hap;
    uint16_t *bk = reinterpret_cast<uint16_t *>(smem + P.lds_off_bk);        // bucket starts [257]
    uint16_t *hpl = reinterpret_cast<uint16_t *>(smem + P.lds_off_hpl);      // haplotype positions grouped by 4-mer
    int *cnt = reinterpret_cast<int *>(smem + P.lds_off_cnt);                // [256] build scratch
    long long *s_item = reinterpret_cast<long long *>(smem + P.lds_off_item);
    // pair area of this 16-lane group
    const int slot = wave * 4 + grp;
    unsigned char *pa = smem + P.lds_shared_bytes + (size_t)slot * P.lds_pair_bytes;
    uint16_t *rd = reinterpret_cast<uint16_t *>(pa + P.lds_off_rd);         // read base | quality index << 8
    double2 *bc = reinterpret_cast<double2 *>(pa + P.lds_off_x);            // [16] the per-base exchange slots
    uint4 *stage = reinterpret_cast<uint4 *>(pa + P.lds_off_x);             // [16] backtrack: 16 back-pointer rows
    int *bm = reinterpret_cast<int *>(pa + P.lds_off_x);                    // [128] coverage bitmap
    int *srt = reinterpret_cast<int *>(pa + P.lds_off_srt);
    // HBM tile of this 16-lane group
    unsigned char *tile = P.ws + P.off_tiles + ((uint64_t)blockIdx.x * DD_FL_PAIRS + (uint64_t)slot) * P.tile_bytes;
    unsigned char *bt = tile;
    int *freq = reinterpret_cast<int *>(tile + P.tile_off_freq);
    int16_t *st = reinterpret_cast<int16_t *>(tile + P.tile_off_freq);     // aliases freq: the histogram is dead once the diagonals are chosen

    for (int i = tid; i < P.n_qual; i += blockDim.x) qt[i] = make_double2(T[T_QUAL + 4 * i], T[T_QUAL + 4 * i + 1]);

    const int32_t *lwin = reinterpret_cast<const int32_t *>(P.ws + DD_LWS_HEADER);
    const int64_t *ioff = reinterpret_cast<const int64_t *>(P.ws + P.off_ioff);
    const int n_lwin = *reinterpret_cast<const int32_t *>(P.ws + DD_LWS_HDR_NWIN);
    const int rounds = *reinterpret_cast<const int32_t *>(P.ws + DD_FL_HDR_ROUNDS);
    const int per_item = rounds * DD_FL_PAIRS;
    const long long n_items = *reinterpret_cast<const int64_t *>(P.ws + DD_FL_HDR_ITEMS);
    unsigned long long my_pairs = 0, my_items = 0;
    int cur_g = -1;

    for (;;) {
        __syncthreads();                                            // the previous item's readers (LDS and s_item) are done
        if (tid == 0) *s_item = (long long)atomicAdd(reinterpret_cast<unsigned long long *>(P.ws + DD_LWS_HDR_COUNTER), 1ull);
        __syncthreads();
        const long long item = *s_item;
        if (item >= n_items) break;
        int jl = 0, jh = n_lwin;                                    // window of the item: last j with ioff[j] <= item
        while (jh - jl > 1) {
            const int mid = (jl + jh) >> 1;
            if (ioff[mid] <= item) jl = mid; else jh = mid;
        }
        const int w = lwin[jl], h0 = P.win_hap_off[w];
        const int r0 = P.win_read_off[w], r1 = P.win_read_off[w + 1], R = r1 - r0;
        const int nsl = (R + per_item - 1) / per_item;
        const int local = (int)(item - ioff[jl]);
        const int g = h0 + local / nsl, s0 = (local % nsl) * per_item;
        const int nslice = (R - s0 < per_item) ? R - s0 : per_item;
        const int hs_off = P.hap_seq_off[g], hlen = P.hap_seq_off[g + 1] - hs_off;
        if (hlen < 1 || hlen > P.max_hap_len) continue;             // guard (the screen never lets such a window in): stays DD_PAIR_UNSUPPORTED
        my_items++;
        const uint32_t hapStart = P.win_hap_start[w];
        const char *hap = P.hap_seq + hs_off;
        const int64_t pair_base = P.win_pair_off[w] + (int64_t)(g - h0) * R;
        const int rs_base = P.read_seq_off[r0];
        const int64_t SL = (int64_t)P.read_seq_off[r1] - rs_base;
        const int64_t hpos_base = P.win_hpos_off[w] + (int64_t)(g - h0) * SL;
        const int nv = P.hap_var_off ? (P.hap_var_off[g + 1] - P.hap_var_off[g]) : 0;
        const bool hap_ok = P.maxLengthDel <= hlen;                 // maxLengthIndel (Faster.cpp:47)
        const int numS = hlen + 2;

        // ---- HapHash (Haplotype.hpp:378-381): positions x < hlen-4 bucketed by their 4-mer; kept while the haplotype stays ----
        if (g != cur_g) {
            cur_g = g;
            for (int i = tid; i < hlen; i += blockDim.x) shHap[i] = (unsigned char)hap[i];
            for (int i = tid; i < 256; i += blockDim.x) cnt[i] = 0;
            __syncthreads();
            for (int hx = tid; hx < hlen - 4; hx += blockDim.x) {
                int key = 0;
                for (int y = 0; y < 4; y++) key |= map_char(shHap[hx + y]) << (2 * y);
                atomicAdd(&cnt[key], 1);
            }
            __syncthreads();
            if (wave == 0) {                                            // exclusive prefix over the 256 buckets
                int c4[4], sum = 0;
                for (int j = 0; j < 4; j++) { c4[j] = cnt[4 * lane + j]; sum += c4[j]; }
                int incl = sum;
                for (int off = 1; off < 64; off <<= 1) {
                    const int o = __shfl_up(incl, off);
                    if (lane >= off) incl += o;
                }
                int run = incl - sum;
                for (int j = 0; j < 4; j++) { bk[4 * lane + j] = (uint16_t)run; cnt[4 * lane + j] = run; run += c4[j]; }
                if (lane == 63) bk[256] = (uint16_t)run;
            }
            __syncthreads();
            for (int hx = tid; hx < hlen - 4; hx += blockDim.x) {
                int key = 0;
                for (int y = 0; y < 4; y++) key |= map_char(shHap[hx + y]) << (2 * y);
                hpl[atomicAdd(&cnt[key], 1)] = (uint16_t)hx;
            }
            __syncthreads();
        }

        // Outputs this model leaves at MLAlignment's defaults, coalesced over the item's pairs.  A pair the reference throws for is finished here.
        for (int t = tid; t < nslice; t += blockDim.x) {
            const int rr = r0 + s0 + t;
            const int L = P.read_seq_off[rr + 1] - P.read_seq_off[rr];
            if (L > P.max_read_len) continue;                              // guard, as above
            const int64_t pair = pair_base + s0 + t;
            const bool good = hap_ok && L >= 4;
            if (P.out.llOn) P.out.llOn[pair] = 0.0;
            if (P.out.llOff) P.out.llOff[pair] = 0.0;
            if (P.out.mLogBQ) P.out.mLogBQ[pair] = 0.0;
            if (P.out.offHap) P.out.offHap[pair] = 0;                          // always false (:491)
            if (P.out.offHapHMQ) P.out.offHapHMQ[pair] = good ? 0 : 1;         // always false (:529); a thrown pair never counts as on-haplotype
            if (P.out.numIndels) P.out.numIndels[pair] = 0;
            if (P.out.numMismatch) P.out.numMismatch[pair] = 0;
            if (P.out.nBQT) P.out.nBQT[pair] = 0;
            if (P.out.nmmBQT) P.out.nmmBQT[pair] = 0;
            if (P.out.nMMLeft) P.out.nMMLeft[pair] = 0;
            if (P.out.nMMRight) P.out.nMMRight[pair] = 0;
            if (!good) {
                P.out.status[pair] = hap_ok ? DD_PAIR_NAN : DD_PAIR_HAPSIZE;
                P.out.ll[pair] = 0.0;
                if (nv > 0) {
                    const int64_t vb = P.win_varcov_off[w] + (int64_t)(P.hap_var_off[g] - P.hap_var_off[h0]) * R + (int64_t)(s0 + t) * nv;
                    for (int i = 0; i < nv; i++) {
                        if (P.out.var_covered) P.out.var_covered[vb + i] = 0;
                        if (P.out.var_fcov) P.out.var_fcov[vb + i] = 0;
                    }
                }
            }
        }
        if (tid == 0) my_pairs += (unsigned long long)nslice;

        for (int rb = 0; rb < nslice; rb += DD_FL_PAIRS) {
            const bool valid = rb + slot < nslice;
            const int ri = s0 + (valid ? rb + slot : 0);
            const int rr = r0 + ri;
            const int64_t pair = pair_base + ri;
            const int so = P.read_seq_off[rr];
            const int Lraw = P.read_seq_off[rr + 1] - so;
            const bool good = valid && hap_ok && Lraw >= 4 && Lraw <= P.max_read_len;
            const int L = good ? Lraw : 0;
            if (__ballot(good) == 0) continue;

            const int bMid = good ? bmid(hapStart, hlen, P.read_start[rr], L) : 0;
            // stage the read, clear the vote histogram (bin index rpfb + L, rpfb in [-(L-4), hlen-5]); 16 bytes = 8 bins per lane and step
            const int F = L + hlen;
            const int nq = good ? ((F + 1) / 2 + 3) / 4 : 0;
            for (int b = l16; b < L; b += 16)
                rd[b] = (uint16_t)((unsigned char)P.read_seq[so + b] | ((unsigned)P.read_qidx[so + b] << 8));
            for (int i = l16; i < nq; i += 16) reinterpret_cast<uint4 *>(freq)[i] = make_uint4(0u, 0u, 0u, 0u);
            wave_sync();
            tile_sync();
            // AlignHash (Faster.cpp:131-189): every read 4-mer votes for the diagonals of the equal haplotype 4-mers
            for (int x = l16; x <= L - 4; x += 16) {
                int key = 0;
                for (int y = 0; y < 4; y++) key |= map_char(rd[x + y] & 0xFF) << (2 * y);
                const int e = bk[key + 1];
                for (int p = bk[key]; p < e; p++) {
                    const int idx = (int)hpl[p] - x + L;
                    atomicAdd(&freq[idx >> 1], (idx & 1) ? 0x10000 : 1);
                }
            }
            // the votes were counted at the L2: wait for them, and let no older copy of the histogram's lines answer the loads below
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            // top 15 diagonals: frequency descending, ties by ascending relative position (:159-181) = descending key
            int myrel = 0x7fffffff;      // lane i < S of the group holds candidate i (unsorted)
            int S = 0;
            bool done = !good;
            unsigned prev = 0xFFFFFFFFu;
            for (int round = 0; round < 15; round++) {
                unsigned best = 0;
                if (!done) {
#pragma unroll 4
                    for (int i = l16; i < nq; i += 16) {
                        const uint4 q = reinterpret_cast<const uint4 *>(freq)[i];
                        const unsigned vv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            const unsigned v = vv[j];
                            const int wi = 4 * i + j;
                            const unsigned f0 = v & 0xFFFFu, f1 = v >> 16;
                            unsigned k0 = f0 ? ((f0 << 16) | (unsigned)(0xFFFF - 2 * wi)) : 0u;
                            unsigned k1 = f1 ? ((f1 << 16) | (unsigned)(0xFFFF - (2 * wi + 1))) : 0u;
                            k0 = k0 < prev ? k0 : 0u;
                            k1 = k1 < prev ? k1 : 0u;
                            const unsigned k = k0 > k1 ? k0 : k1;
                            best = k > best ? k : best;
                        }
                    }
                }
#pragma unroll
                for (int off = 8; off >= 1; off >>= 1) {
                    const unsigned o = __shfl_xor(best, off, 16);
                    best = o > best ? o : best;
                }
                done = done || best == 0;
                if (!done) {
                    const int idx = 0xFFFF - (int)(best & 0xFFFFu);
                    if (l16 == S) myrel = idx - L;
                    prev = best;
                    S++;
                }
                if (__ballot(!done) == 0) break;
            }
            if (good) {
                if (l16 == S) myrel = -L;                // relPos.push_back(-readLen) (:263)
                S++;
            }
            // sort ascending (values are distinct): rank = number of smaller values
            srt[l16] = myrel;
            wave_sync();
            int rank = 0;
#pragma unroll
            for (int i = 0; i < 16; i++) rank += (srt[i] < myrel) ? 1 : 0;
            wave_sync();
            srt[l16 < S ? rank : l16] = (l16 < S) ? myrel : 0;
            wave_sync();
            const int relMine = srt[l16];
            const bool act = good && l16 < S;
            const int Smax = gmax4(S);
#include "faster_sstate.inc"   // SStateHMM (:253-576): sweeps and join; defines ll and xH
            // backtrack (:540-548); every lane of the group walks the same path.  code = diagonal | 16 if inserted.  The rows come
            // from the tile 16 at a time (one 16-byte row per lane) through the scratch X, the next 16 already in flight; lane i keeps
            // the state of row 16 c + i, so the path goes out 32 bytes at a time.
            tile_sync();                                             // the rows are written; X's exchange slots and the histogram are dead
            const uint4 *bt4 = reinterpret_cast<const uint4 *>(bt);
            if (l16 == 0 && good) st[bMid] = (int16_t)xH;
            {   // rows bMid-1 .. 0
                const int nch = good ? (bMid + 15) >> 4 : 0;
                const int iters = gmax4(nch);
                int code = xH;
                uint4 nxt = make_uint4(0u, 0u, 0u, 0u);
                if (nch > 0 && (nch - 1) * 16 + l16 < bMid) nxt = bt4[(nch - 1) * 16 + l16];
                for (int it = 0; it < iters; it++) {
                    const int ci = nch - 1 - it;
                    wave_sync();
                    stage[l16] = nxt;
                    wave_sync();
                    if (ci >= 1) nxt = bt4[(ci - 1) * 16 + l16];
                    int mine = 0;
                    const unsigned char *sb = reinterpret_cast<const unsigned char *>(stage);
#pragma unroll 4
                    for (int i = 15; i >= 0; i--) {
                        if (ci >= 0 && ci * 16 + i < bMid) {
                            const int d = code & 15, wv = sb[i * 16 + d];
                            if (code & 16) code = (wv & 32) ? 0 : (d | (wv & 16));
                            else { const int c = wv & 15; code = c | (c > d ? 16 : 0); }
                            mine = (l16 == i) ? code : mine;
                        }
                    }
                    if (ci >= 0 && ci * 16 + l16 < bMid) st[ci * 16 + l16] = (int16_t)mine;
                }
            }
            {   // rows bMid+1 .. L-1
                const int c0 = (bMid + 1) >> 4;
                const int nch = (good && bMid < L - 1) ? ((L - 1) >> 4) - c0 + 1 : 0;
                const int iters = gmax4(nch);
                int code = xH;
                uint4 nxt = make_uint4(0u, 0u, 0u, 0u);
                if (nch > 0 && c0 * 16 + l16 < L) nxt = bt4[c0 * 16 + l16];
                for (int it = 0; it < iters; it++) {
                    const int ci = c0 + it;
                    const bool cact = it < nch;
                    wave_sync();
                    stage[l16] = nxt;
                    wave_sync();
                    if (it + 1 < nch && (ci + 1) * 16 + l16 < L) nxt = bt4[(ci + 1) * 16 + l16];
                    int mine = 0;
                    const unsigned char *sb = reinterpret_cast<const unsigned char *>(stage);
#pragma unroll 4
                    for (int i = 0; i < 16; i++) {
                        const int b1 = ci * 16 + i;
                        if (cact && b1 > bMid && b1 < L) {
                            const int d = code & 15, wv = sb[i * 16 + d];
                            const int wd = 32 - __clz(d + 1);
                            if (code & 16) { const int ii = wv & ((1 << wd) - 1); code = ii == 0 ? 0 : (ii == 1 ? (d | 16) : ii - 2); }
                            else { const int n = wv >> wd; code = n == 0 ? 0 : (n == 1 ? (d | 16) : n - 2 + d); }
                            mine = (l16 == i) ? code : mine;
                        }
                    }
                    const int bs = ci * 16 + l16;
                    if (cact && bs > bMid && bs < L) st[bs] = (int16_t)mine;
                }
            }
            tile_sync();
            // mapState (:552-571) and reportVariants (:579-681: hpos, firstBase / lastBase), 16 bases at a time.  lhp — the last haplotype
            // position + 1 an on-diagonal base mapped to, 1 before the first — is a running "last defined value": a scan inside the 16
            // lanes, carried from one 16 bases to the next.
            int firstB = 0x7fffffff, lastB = -1;
            int16_t *hp_out = (P.out.hpos && good) ? P.out.hpos + hpos_base + (so - rs_base) : nullptr;
            {
                const int iters = gmax4((L + 15) >> 4);
                int lhp = 1;
                int cnx = (l16 < L) ? st[l16] : 0;
                for (int it = 0; it < iters; it++) {
                    const int r = it * 16 + l16;
                    const bool in = r < L;
                    const int c = cnx;
                    if (r + 16 < L) cnx = st[r + 16];
                    int v = -1, m = 0;
                    if (in && !(c & 16)) {
                        const int hp = srt[c & 15] + r;
                        if (hp >= 0 && hp < hlen) { m = hp + 1; v = hp + 1; }
                        else if (hp < 0) m = 0; else m = hlen;
                    }
#pragma unroll
                    for (int off = 1; off < 16; off <<= 1) {
                        const int o = __shfl_up(v, off, 16);
                        v = (l16 >= off && v < 0) ? o : v;
                    }
                    const int lh = v >= 0 ? v : lhp;
                    if (in && (c & 16)) m = hlen + 2 + lh;
                    lhp = __shfl(lh, 15, 16);
                    if (in) {
                        st[r] = (int16_t)m;                            // the coverage test below reads it
                        const int s = m;
                        const int xm = s % numS;
                        int hp;
                        if (xm > 0 && xm <= hlen) {
                            if (s >= numS) hp = DD_HPOS_INS_KEY0 - xm;     // inserted base, carrying its key (pos = lhp, :556-566, :608)
                            else { hp = s - 1; firstB = hp < firstB ? hp : firstB; lastB = hp > lastB ? hp : lastB; }
                        } else hp = (xm == 0) ? DD_HPOS_LO : DD_HPOS_RO;
                        if (hp_out) hp_out[r] = (int16_t)hp;
                    }
                }
            }
#define FAST_ST_VISIBLE() tile_sync()   /* st is in the tile */
#include "faster_pair_end.inc"   // firstBase / lastBase, var_covered, var_fcov, the final store
            wave_sync();
            tile_sync();                                      // the tile's readers are done before the next pair clears it
        }
    }
    if (tid == 0 && my_items) {
        atomicAdd(&P.stats[0], my_pairs);
        atomicMax(&P.stats[1], my_pairs);
        atomicMax(&P.stats[2], my_items);
    }
}

// onHap[r] of the long windows' reads, after the kernel (kernel_common.h)
__global__ void dd_faster_long_onhap_kernel(const FLArgs P) { ddc::onhap_of_read(P); }

size_t fl_lds_layout(int max_hap_len, int max_read_len, FLArgs &A)
{
    uint32_t off = 0;
    A.lds_off_qt = off;   off = up16(off + 16u * (uint32_t)(A.n_qual > 0 ? A.n_qual : 1));
    A.lds_off_hap = off;  off = up16(off + (uint32_t)max_hap_len);
    A.lds_off_bk = off;   off = up16(off + 2u * 257u);
    A.lds_off_hpl = off;  off = up16(off + 2u * (uint32_t)max_hap_len);
    A.lds_off_cnt = off;  off = up16(off + 4u * 256u);
    A.lds_off_item = off; off = up16(off + 16u);
    A.lds_shared_bytes = off;
    uint32_t po = 0;
    A.lds_off_rd = po;  po = up16(po + 2u * (uint32_t)max_read_len);
    A.lds_off_x = po;   po = up16(po + 512u);           // 16 double2 exchange slots / 16 staged rows / 128 bitmap words (4,094 bp)
    A.lds_off_srt = po; po = up16(po + 64u);
    A.lds_pair_bytes = po;
    return (size_t)off + (size_t)DD_FL_PAIRS * po;
}

uint64_t fl_tile_layout(int max_hap_len, int max_read_len, FLArgs &A)
{
    auto al = [](uint64_t v) { return (v + 255u) & ~(uint64_t)255u; };
    A.tile_off_freq = al(16u * (uint64_t)max_read_len);
    A.tile_bytes = A.tile_off_freq + al(4u * (uint64_t)((max_hap_len + max_read_len + 1) / 2 + 4));
    return A.tile_bytes;
}

hipError_t launch_faster_long(const FLArgs &A, unsigned grid, size_t lds, bool onhap, hipStream_t st)
{
    if (grid < 1) return hipErrorInvalidValue;
    // the dynamic-LDS cap is raised once per device, as for the other kernels
    static std::atomic<unsigned> raised(0u);
    hipError_t e = ddc::raise_lds_cap_once(reinterpret_cast<const void *>(&dd_faster_long_kernel), raised);
    if (e != hipSuccess) return e;
    if (lds > 160u * 1024u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dd_faster_long_prepass, dim3(1), dim3(1024), 0, st, A);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dd_faster_long_kernel, dim3(grid), dim3(DD_FL_THREADS), lds, st, A);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (onhap && A.read_end > A.read_begin) {
        hipLaunchKernelGGL(dd_faster_long_onhap_kernel, dim3((A.read_end - A.read_begin + 255) / 256), dim3(256), 0, st, A);
        e = hipGetLastError();
    }
    return e;
}

} // namespace ddf
