// long_kernel.hip — gfx950 kernel for the windows the main kernels do not cover: haplotypes of 767..4,094 bp, reads of
// 1,025..4,096 bp, and (maxLengthDel 12..31) haplotypes of 575..766 bp.  Runs as a launch of its own, after the main launch, and
// overwrites the placeholder outputs of its windows (dd_launch_device_long, dd_compute_likelihoods_ex).
//
// Per (haplotype, read) pair it computes what the main kernel's generic code path computes (hmm_kernel.hip, the LEAN / BIGD parts:
// jump candidates in a run-time loop over y), ObservationModelFBMaxErr::calcLikelihood (reference ObservationModelFB.cpp:1057-1165,
// 1351-1475, 1641-1829), with the same fp64 sums in the same term order, no transcendental on the device (tables from dd_build_tables)
// and the full pass with RO always evaluated (no speculative skip).
//
// Mapping:
//   * one workgroup of 256 threads = one pair at a time; a persistent grid draws pairs from a counter in the workspace header;
//   * thread t owns the K states x = k * 256 + t (k < K, numS = Hs + 2 <= 256 K): a read base is one sweep over those, the neighbours'
//     values come from a workgroup LDS row {alpha/beta, emission} (+ the inserted states' row in the left->middle pass); two barriers
//     per read base (row published / row read);
//   * back-pointers: one byte per (read base, state) — 6 bits of transition choice (jump length y <= 32, 0 = inserted state; LO / RO
//     codes as in the main kernel) + 1 bit for the inserted state — in a per-workgroup HBM tile of max_read_len x 256 K bytes (followed by
//     2 x 256 K doubles where K = 16 parks beta[bMid]);
//   * the join's arg max is a workgroup max + count of near-ties; with more than one state within 3e-10 the reference's scan is replayed
//     serially (hmm_kernel.hip slice_argmax);
//   * traceback, hpos, QC counters and coverage flags run on wavefront 0 from the tile and LDS, with the main kernel's run detection.
// The wide build (maxLengthDel above 31, opt-in: DD_OPT_WIDE_DELETIONS) is the same kernel with two bytes per back-pointer
// (12 bits of choice: jump lengths up to 4,095) and its candidate loops clipped to the haplotype; it runs without a main launch in front,
// so its launch writes the placeholders of the screened windows and onHap of every read itself.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include "hmm_kernel.h"
#include "kernel_common.h"
#include "long_kernel.h"

namespace ddl {
using ddc::up16;

#define LNEG_INF (-__builtin_huge_val())
#define L_EPS 1e-10
constexpr int NT = DD_LONG_THREADS;
constexpr int PAD = DD_LONG_PAD;
// a back-pointer field: choice bits (jump lengths 0..32; the wide build's 0..4095), then one bit for the inserted state
constexpr int choice_bits(bool wide) { return wide ? 12 : 6; }
constexpr unsigned ins_bit(bool wide) { return 1u << choice_bits(wide); }
constexpr unsigned choice_mask(bool wide) { return ins_bit(wide) - 1u; }
constexpr unsigned field_mask(bool wide) { return (ins_bit(wide) << 1) - 1u; }
template <bool WIDE> struct BtField { typedef unsigned char type; };      // the field as it lies in the tile
template <> struct BtField<true> { typedef uint16_t type; };
constexpr int HP_DEF = 64;                             // E/N code of a state without a homopolymer entry: log(1e-5), log(1-1e-5)
constexpr int SYM_N = 4, SYM_PAD = 255;

__device__ __forceinline__ double dmax(double a, double b)
{
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

__device__ __forceinline__ int builtin_symbol(unsigned ch)
{
    return ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : ch == 'N' ? SYM_N : 31;
}

// bit c set <=> a state with symbol `code` emits "eq" for read symbol c ('N' / LO / RO: every column; a pad: none)
__device__ __forceinline__ unsigned sym_mask(unsigned code)
{
    return code == (unsigned)SYM_N ? 0xffffffffu : (code < 32u ? 1u << code : 0u);
}

__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}

// workgroup max (plain max, the reference's llOn); every thread gets it.  red: 4 doubles of LDS
__device__ __forceinline__ double block_max(double v, double *red)
{
    const int t = threadIdx.x;
    v = wave_max(v);
    if ((t & 63) == 0) red[t >> 6] = v;
    __syncthreads();
    double m = red[0];
#pragma unroll
    for (int i = 1; i < NT / 64; i++) m = red[i] > m ? red[i] : m;
    __syncthreads();
    return m;
}

// arg max over the join slice with the reference's scan semantics (ObservationModelFB.cpp:1096-1102, 1110-1114): states in index order
// (on-base 0..numS-1, then inserted numS..2 numS-1), a state replaces the incumbent only if it beats it by more than EPS.  One state within
// 3e-10 of the maximum: the scan provably ends on it.  Otherwise the scan is replayed verbatim from LDS by one thread.
template <int K>
__device__ void block_argmax(const double (&vA)[K], const double (&vI)[K], int numS, double *scan, double *red, int *redi,
                             double &best, int &idx)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double m = LNEG_INF;
#pragma unroll
    for (int k = 0; k < K; k++) {
        m = vA[k] > m ? vA[k] : m;
        m = vI[k] > m ? vI[k] : m;
    }
    m = block_max(m, red);
    const double thr = m - 3e-10;
    int cnt = 0, cand = -1;
#pragma unroll
    for (int k = 0; k < K; k++) {
        const int x = k * NT + t;
        if (vA[k] >= thr) { cnt++; cand = x; }
        if (vI[k] >= thr) { cnt++; cand = numS + x; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        cnt += __shfl_xor(cnt, off);
        const int oc = __shfl_xor(cand, off);
        cand = oc > cand ? oc : cand;
    }
    if (lane == 0) { redi[wave] = cnt; redi[4 + wave] = cand; }
    __syncthreads();
    int total = 0, c = -1;
#pragma unroll
    for (int i = 0; i < NT / 64; i++) { total += redi[i]; c = redi[4 + i] > c ? redi[4 + i] : c; }
    if (total == 1) {
        best = m; idx = c;
        __syncthreads();                               // redi is reused by the next call
        return;
    }
#pragma unroll
    for (int k = 0; k < K; k++) {
        const int x = k * NT + t;
        if (x < numS) { scan[x] = vA[k]; scan[numS + x] = vI[k]; }
    }
    __syncthreads();
    if (t == 0) {
        double b = LNEG_INF;
        int ix = 0;
        for (int s = 0; s < 2 * numS; s++) {
            const double v = scan[s];
            if (v > b + L_EPS) { b = v; ix = s; }
        }
        red[0] = b; redi[0] = ix;
    }
    __syncthreads();
    best = red[0]; idx = redi[0];
    __syncthreads();
}

// The long windows of [w_begin, w_end) in order, and the prefix sums of their pair counts (kernel_common.h)
__global__ void __launch_bounds__(1024) dd_long_prepass(const LongArgs P)
{
    __shared__ int32_t sc[1024];
    __shared__ long long sp[1024];
    const long long total = ddc::long_prepass(P, P.off_lpoff, 2, sc, sp, [&](int w) { return (long long)(P.win_pair_off[w + 1] - P.win_pair_off[w]); });
    if (threadIdx.x == 1023) *reinterpret_cast<int64_t *>(P.ws + DD_LONG_HDR_TOTAL) = total;
}

// WIDE (maxLengthDel > 31, DD_OPT_WIDE_DELETIONS): 16-bit back-pointer fields, and candidate loops clipped to the haplotype instead of
// running into the row pads (the clipped-away candidates are the reference's clamped sources, which never win)
template <int K, bool WIDE>
__global__ void __launch_bounds__(NT, K >= 16 ? 1 : 2) dd_long_kernel(const LongArgs P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NP = NT * K;
    constexpr int CB = choice_bits(WIDE);
    constexpr unsigned INS_BIT = ins_bit(WIDE), CHMASK = choice_mask(WIDE), FMASK = field_mask(WIDE);
    typedef typename BtField<WIDE>::type bt_t;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double2 *rowA = reinterpret_cast<double2 *>(smem);                        // [PAD + NP + PAD] state s at PAD + s: {alpha / beta, emission}
    double *rowI = reinterpret_cast<double *>(smem + P.lds_off_rowI);          // [1 + NP]  inserted state s at 1 + s
    unsigned char *sc = smem + P.lds_off_sc;                                   // [NP] state symbols
    unsigned char *hc = smem + P.lds_off_hc;                                   // [NP + 2 PAD] E/N code per state (index into shEN)
    double2 *shEN = reinterpret_cast<double2 *>(smem + P.lds_off_EN);          // [65] {logProbError, logProbNoError}
    double *shQ = reinterpret_cast<double *>(smem + P.lds_off_Q);              // [n_qual][4] eq, uq, log10(1-q), q
    unsigned char *shLut = smem + P.lds_off_lut;                               // [256]
    unsigned char *rdC = smem + P.lds_off_rdC;                                 // [Lmax] read symbol
    unsigned char *rdQ = smem + P.lds_off_rdQ;                                 // [Lmax] quality index
    int16_t *ms = reinterpret_cast<int16_t *>(smem + P.lds_off_ms);            // [Lmax] MAP state per read base
    double *red = reinterpret_cast<double *>(smem + P.lds_off_red);            // [64] reductions / mLogBQ terms
    int *redi = reinterpret_cast<int *>(red + 64);                             // [16]: [0, 8) reductions, [12, 16) the drawn item
    long long *s_item = reinterpret_cast<long long *>(redi + 12);

    const double *T = P.tables;
    const double lLL = T[TC_LLL], lFL = T[TC_LFL], II = T[TC_II], NI = T[TC_NI], NN = T[TC_NN];
    for (int i = t; i < 4 * P.n_qual; i += NT) shQ[i] = T[T_QUAL + i];
    for (int i = t; i < 256; i += NT) shLut[i] = P.sym_lut ? P.sym_lut[i] : (unsigned char)builtin_symbol((unsigned)i);
    for (int i = t; i <= HP_DEF; i += NT)
        shEN[i] = i < HP_DEF ? make_double2(T[T_HP + 2 * i], T[T_HP + 2 * i + 1]) : make_double2(T[TC_EDEF], T[TC_NDEF]);

    unsigned long long *counter = reinterpret_cast<unsigned long long *>(P.ws + DD_LWS_HDR_COUNTER);
    const int n_long = *reinterpret_cast<const int32_t *>(P.ws + DD_LWS_HDR_NWIN);
    const long long total = *reinterpret_cast<const int64_t *>(P.ws + DD_LONG_HDR_TOTAL);
    const int32_t *lwin = reinterpret_cast<const int32_t *>(P.ws + DD_LWS_HEADER);
    const int64_t *lpoff = reinterpret_cast<const int64_t *>(P.ws + P.off_lpoff);
    unsigned char *tile = P.ws + P.off_tiles + (size_t)blockIdx.x * P.tile_bytes;
    unsigned long long my_pairs = 0;

    for (;;) {
        __syncthreads();                               // the previous pair's LDS and tile are no longer read
        if (t == 0) *s_item = (long long)atomicAdd(counter, 1ull);
        __syncthreads();
        const long long item = *s_item;
        if (item >= total) break;
        my_pairs++;
        // window of the item: the last j with lpoff[j] <= item
        int lo = 0, hi = n_long;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (lpoff[mid] <= item) lo = mid; else hi = mid;
        }
        const int w = lwin[lo];
        const long long local = item - lpoff[lo];
        const int h0 = P.win_hap_off[w];
        const int r0 = P.win_read_off[w], r1 = P.win_read_off[w + 1];
        const int R = r1 - r0;
        const int hi_ = (int)(local / R), ri = (int)(local - (long long)hi_ * R);
        const int g = h0 + hi_, r = r0 + ri;
        const int64_t pair = P.win_pair_off[w] + local;
        const int hs_off = P.hap_seq_off[g];
        const int Hs = P.hap_seq_off[g + 1] - hs_off;
        const int numS = Hs + 2, RO = Hs + 1;
        const int so = P.read_seq_off[r];
        const int L = P.read_seq_off[r + 1] - so;
        const uint32_t hapStart = P.win_hap_start[w];
        const int nv = P.hap_var_off ? (P.hap_var_off[g + 1] - P.hap_var_off[g]) : 0;
        const int64_t vb = nv > 0 ? P.win_varcov_off[w] + (int64_t)(P.hap_var_off[g] - P.hap_var_off[h0]) * R + (int64_t)ri * nv : 0;
        if (L < 1 || Hs < 1 || L > P.max_read_len || numS > NP) {
            // outside what this launch was sized for (a caller's maxima that do not cover the batch): marked, nothing written out of bounds
            if (t == 0) {
                P.out.status[pair] = DD_PAIR_UNSUPPORTED;
                P.out.ll[pair] = 0.0;
                if (P.out.offHap) P.out.offHap[pair] = 1;
                if (P.out.offHapHMQ) P.out.offHapHMQ[pair] = 1;
            }
            continue;
        }
        if (P.maxLengthDel > Hs) {                     // "hapSize error." (ObservationModelFB.cpp:47): status, no coverage flags
            if (t == 0) { P.out.status[pair] = DD_PAIR_HAPSIZE; P.out.ll[pair] = 0.0; }
            for (int i = t; i < nv; i += NT) {
                if (P.out.var_covered) P.out.var_covered[vb + i] = 0;
                if (P.out.var_fcov) P.out.var_fcov[vb + i] = 0;
            }
            continue;
        }

        // ---- per-pair setup: state symbols, homopolymer indel-error codes (setupTransitionProbs :1675-1703), the read, the row pads
        const char *hp = P.hap_seq + hs_off;
        for (int s = t; s < NP + 2 * PAD; s += NT) {
            if (s < NP) {
                int code = SYM_PAD;
                if (s == 0 || s == RO) code = SYM_N;
                else if (s < RO) code = shLut[(unsigned char)hp[s - 1]];
                sc[s] = (unsigned char)code;
            }
            hc[s] = HP_DEF;
        }
        for (int b = t; b < L; b += NT) {
            rdC[b] = shLut[(unsigned char)P.read_seq[so + b]];
            rdQ[b] = P.read_qidx[so + b];
        }
        for (int i = t; i < PAD; i += NT) {
            rowA[i] = make_double2(LNEG_INF, 0.0);
            rowA[PAD + NP + i] = make_double2(LNEG_INF, 0.0);
        }
        if (t == 0) rowI[0] = LNEG_INF;
        __syncthreads();
        if (t == 0) hc[1] = 1;
        __syncthreads();
        for (int b = 1 + t; b < Hs; b += NT) {
            if (hp[b] != hp[b - 1]) {
                int len = 1;
                while (b - 1 - len >= 0 && hp[b - 1 - len] == hp[b - 1]) len++;
                hc[b] = (unsigned char)(len < DD_HP_TABLE - 1 ? len : DD_HP_TABLE - 1);
            }
        }
        __syncthreads();
        if (t == 0) {
            int len = 1;
            while (Hs - 1 - len >= 0 && hp[Hs - 1 - len] == hp[Hs - 1]) len++;
            hc[Hs - 1] = (unsigned char)(len < DD_HP_TABLE - 1 ? len : DD_HP_TABLE - 1);   // index hapSize-1, as the reference writes it (:1702)
        }
        __syncthreads();
        const int Dr = P.D;
        const double Nn_RO = shEN[hc[RO]].y, E_RO = shEN[hc[RO]].x, E_Hs = shEN[hc[Hs]].x, E_1 = shEN[hc[1]].x;

        // ---- bMid: ObservationModelFB::Init (:51-99) ----
        int bMid;
        {
            const uint32_t hapEnd = hapStart + (uint32_t)Hs;
            const uint32_t mReadStart = P.read_start[r];
            const uint32_t readEnd = mReadStart + (uint32_t)L - 1u;
            if ((P.read_flags[r] & 1) || mReadStart > hapEnd || readEnd < hapStart) {
                bMid = L / 2;
            } else {
                const uint32_t olStart = (hapStart > mReadStart) ? hapStart : mReadStart;
                const uint32_t olEnd = (hapEnd > readEnd) ? readEnd : hapEnd;
                const int mid = ((int)olEnd - (int)olStart) / 2 + (int)olStart;
                bMid = mid - (int)mReadStart;
            }
            if (P.bMid != -1) bMid = P.bMid;
            if (bMid < 0) bMid = 0;
            if (bMid >= L) bMid = L - 1;
        }

        // beta[bMid] waits for the join in registers — or, at K = 16 (whose 2 x 16 doubles of it would push the kernel past 256 VGPRs), behind
        // the workgroup's back-pointer tile in HBM: the thread that stores a value loads it back
        constexpr bool STASH = K >= 16;
        double a[K], in[K], be_a[STASH ? 1 : K], be_i[STASH ? 1 : K];
        double *beS = reinterpret_cast<double *>(tile + P.stash_off);
        // ================= right -> middle: passMessageTwoInc for b = L-1..bMid+1 (:1576-1578, :1715-1773)
#pragma unroll
        for (int k = 0; k < K; k++) {
            const bool valid = k * NT + t < numS;
            a[k] = valid ? 0.0 : LNEG_INF;             // beta[L-1][*] = 0
            in[k] = valid ? 0.0 : LNEG_INF;
        }
        for (int b = L - 1; b > bMid; b--) {
            const int qi = rdQ[b];
            const double eq = shQ[4 * qi], uq = shQ[4 * qi + 1];
            const int col = rdC[b];
#pragma unroll
            for (int k = 0; k < K; k++) {
                const int x = k * NT + t;
                rowA[PAD + x] = make_double2(a[k], ((sym_mask(sc[x]) >> col) & 1u) ? eq : uq);
            }
            __syncthreads();
            bt_t *trow = reinterpret_cast<bt_t *>(tile) + (size_t)b * NP;
#pragma unroll
            for (int k = 0; k < K; k++) {
                const int x = k * NT + t;
                const double2 s1 = rowA[PAD + x + 1];  // state x+1
                double best;
                {
                    double c = LNEG_INF;
                    if (x + 1 <= RO) { const double Ns = shEN[hc[x + 1]].y; c = Ns + Ns; }     // lp + Nn[src], y = 1 (:1730-1735)
                    best = (c + s1.x) + s1.y;
                }
                unsigned ch = 1;
                const int yEnd = WIDE ? min(Dr, RO - x) : Dr;  // wide: sources up to RO only
#pragma unroll 1
                for (int y = 2; y <= yEnd; y++) {
                    const int src = x + y;
                    const double yII = (double)(y - 1) * II;
                    const double2 tv = rowA[PAD + src];
                    double c = LNEG_INF;
                    if (src <= RO) { const double2 en = shEN[hc[src]]; c = (en.x + yII) + en.y; }
                    const double val = (c + tv.x) + tv.y;
                    const bool take = val > best + L_EPS;    // newIdx > destIdx: branch 1 only
                    best = take ? val : best;
                    ch = take ? (unsigned)y : ch;
                }
                {
                    const double eInc = (x + 1 <= RO) ? shEN[hc[x + 1]].x : LNEG_INF;
                    const double val = (eq + in[k]) + eInc;  // to inserted state numS+x (:1746-1749)
                    if (val > best + L_EPS) { best = val; ch = 0; }
                }
                double na = best;
                const double d = (eq + in[k]) + II;           // (:1754-1758)
                const double v2 = (s1.y + s1.x) + NI;         // src = x+1 (:1763-1767)
                const bool tk = v2 >= d;
                const double ni = dmax(d, v2);
                unsigned code = ch | (tk ? INS_BIT : 0u);
                if (x == 0) {                                 // LO (:1720-1722, :1746-1749, :1762)
                    double bst = ((eq + a[k]) + lLL) + NN;
                    unsigned cd = 0;
                    const double c2 = ((s1.y + s1.x) + lFL) + NN;
                    if (c2 > bst + L_EPS) { bst = c2; cd = 1; }
                    const double c3 = (eq + in[k]) + E_1;
                    if (c3 > bst + L_EPS) { bst = c3; cd = 2; }
                    na = bst;
                    const double vv = (eq + a[k]) + NI;
                    code = cd | ((vv >= d) ? INS_BIT : 0u);
                    in[k] = dmax(d, vv);
                } else if (x == RO) {                         // RO (:1741-1742, :1750, :1763-1767)
                    double bst = (eq + a[k]) + Nn_RO;
                    unsigned cd = 0;
                    const double c2 = eq + in[k];
                    if (c2 > bst + L_EPS) { bst = c2; cd = 1; }
                    na = bst;
                    const double vv = (eq + a[k]) + NI;
                    code = cd | ((vv >= d) ? INS_BIT : 0u);
                    in[k] = dmax(d, vv);
                } else {
                    in[k] = ni;
                }
                a[k] = na;
                trow[x] = (bt_t)code;                // btb[b-1] stored at row b
            }
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < K; k++) {                  // beta[bMid]
            if constexpr (STASH) { beS[k * NT + t] = a[k]; beS[NP + k * NT + t] = in[k]; }
            else { be_a[k] = a[k]; be_i[k] = in[k]; }
        }

        // ================= left -> middle: passMessageTwoDec for b = 1..bMid (:1573-1575, :1775-1829), RO evaluated
#pragma unroll
        for (int k = 0; k < K; k++) {
            const bool valid = k * NT + t < numS;
            a[k] = valid ? 0.0 : LNEG_INF;             // alpha[0][*] = 0 (:335-338)
            in[k] = valid ? 0.0 : LNEG_INF;
        }
        for (int b = 1; b <= bMid; b++) {
            const int qi = rdQ[b - 1];
            const double eq = shQ[4 * qi], uq = shQ[4 * qi + 1];
            const int col = rdC[b - 1];
            double ovo[K];
#pragma unroll
            for (int k = 0; k < K; k++) {
                const int x = k * NT + t;
                ovo[k] = ((sym_mask(sc[x]) >> col) & 1u) ? eq : uq;
                rowA[PAD + x] = make_double2(a[k], ovo[k]);
                rowI[1 + x] = in[k];
            }
            __syncthreads();
            bt_t *trow = reinterpret_cast<bt_t *>(tile) + (size_t)b * NP;
#pragma unroll
            for (int k = 0; k < K; k++) {
                const int x = k * NT + t;
                const bool valid = x < numS;
                const double2 en = shEN[hc[x]];
                const double lpn = valid ? en.y : LNEG_INF;   // logProbNoError[x]
                const double eIn = valid ? en.x : LNEG_INF;   // logProbError[x]
                const double niDec = (x == 0) ? LNEG_INF : NI;
                const double2 s1 = rowA[PAD + x - 1];          // state x-1 (the left pad below state 0)
                double best = ((s1.y + lpn) + s1.x) + lpn;     // (:1793), y = 1
                unsigned ch = 1;
                const int yEnd = WIDE ? min(Dr, x) : Dr;       // wide: sources down to LO only
#pragma unroll 1
                for (int y = 2; y <= yEnd; y++) {
                    const double2 tv = rowA[PAD + x - y];
                    const double lp = eIn + (double)(y - 1) * II;
                    const double val = ((tv.y + lp) + tv.x) + lpn;
                    const bool take = val >= best;             // newIdx < destIdx: either branch of updateMax
                    best = dmax(best, val);
                    ch = take ? (unsigned)y : ch;
                }
                const double ip = rowI[x];                     // inserted state numS+x-1
                {
                    const double val = (eq + ip) + eIn;        // (:1807-1811)
                    if (val > best + L_EPS) { best = val; ch = 0; }
                }
                double na = best;
                const double d = (eq + in[k]) + II;            // stay inserted (:1816-1820)
                const double v2 = (ovo[k] + a[k]) + niDec;     // open insertion after x (:1823-1826)
                const bool tk = v2 >= d;
                const double ni = dmax(d, v2);
                unsigned code = ch | (tk ? INS_BIT : 0u);
                if (x == 0) {                                  // (:1798-1799)
                    na = (eq + a[k]) + NN;
                    code = 0;
                } else if (x == RO) {                          // (:1780-1782, :1804-1805)
                    const double aHs = s1.x, oHs = s1.y, iHs = ip;
                    double bst = ((eq + a[k]) + lLL) + NN;
                    unsigned cd = 0;
                    const double c2 = ((oHs + aHs) + lFL) + NN;
                    const bool t2 = c2 >= bst;                 // smaller index: either branch
                    bst = dmax(bst, c2);
                    cd = t2 ? 1u : cd;
                    const double c3 = ((eq + in[k]) + lLL) + E_RO;
                    const bool t3 = c3 > bst + L_EPS;          // larger index: branch 1 only
                    bst = t3 ? c3 : bst;
                    cd = t3 ? 2u : cd;
                    const double c4 = ((eq + iHs) + lFL) + E_Hs;
                    const bool t4 = (c4 > bst + L_EPS) || (t3 && c4 >= bst);   // numS+Hs < numS+RO only
                    bst = t4 ? c4 : bst;
                    cd = t4 ? 3u : cd;
                    na = bst;
                    code = (code & INS_BIT) | cd;
                }
                a[k] = na;
                in[k] = ni;
                trow[x] = (bt_t)code;
            }
            __syncthreads();
        }

        // ================= join at bMid: calcLikelihoodFromLastSlice (:1075-1144) + computeBMidPrior (:268-305)
        double ll, llHMQ, llOff = LNEG_INF, llOn;
        int mapRMQ, mapHMQ;
        {
            const int qi = rdQ[bMid];
            const double eq = shQ[4 * qi], uq = shQ[4 * qi + 1];
            const int col = rdC[bMid];
            const int mqi = P.read_mqidx[r];
            const double prOff0 = T[T_MAPQ + 4 * mqi + 0], prOff1 = T[T_MAPQ + 4 * mqi + 1];
            const double prOn0 = T[T_MAPQ + 4 * mqi + 2], prOn1 = T[T_MAPQ + 4 * mqi + 3];
            const double hqOff0 = T[TC_HMQ + 0], hqOff1 = T[TC_HMQ + 1], hqOn0 = T[TC_HMQ + 2], hqOn1 = T[TC_HMQ + 3];
            const double roPrior = -100.0;                     // prior[RO] (:299)
            bool usePin = false;
            int pinBase = 0, pinMax = 1, pinD0 = 0;
            if (P.read_mate_pos) {
                const int fl = P.read_flags[r], mlen = P.read_mate_len[r];
                usePin = (fl & DD_READ_PAIRED) && !(fl & DD_READ_MATE_UNMAPPED) && mlen != -1 && (fl & DD_READ_MATE_SAME_TID);
                if (usePin) {
                    const int lib = P.read_lib[r];
                    pinBase = P.lib_off[lib];
                    pinMax = P.lib_off[lib + 1] - pinBase;
                    pinD0 = (fl & DD_READ_MATE_REVERSE) ? (int)hapStart - bMid - (P.read_mate_pos[r] + mlen)
                                                        : (int)hapStart + L - bMid - P.read_mate_pos[r];
                }
            }
            const double lpOffR = T[T_MAPQ2 + 2 * mqi], lpOnR = T[T_MAPQ2 + 2 * mqi + 1];
            const double lpOffH = T[TC_PINS + 1], lpOnH = T[TC_PINS + 2];
            const double lIns0 = T[TC_PINS + 0], lIns1 = T[TC_IN];
            const double pin0 = usePin ? P.lib_log95[P.read_lib[r]] : 0.0;
            // priors of join state x (computeBMidPrior :296-303): the read's mapping quality (hmq = false) or 1-1e-10 (:1093, hmq = true)
            auto priors = [&](int x, bool hmq, double &p0, double &p1) __attribute__((always_inline)) {
                if (x == RO) { p0 = p1 = roPrior; return; }
                if (!usePin) {
                    if (x == 0) { p0 = hmq ? hqOff0 : prOff0; p1 = hmq ? hqOff1 : prOff1; }
                    else { p0 = hmq ? hqOn0 : prOn0; p1 = hmq ? hqOn1 : prOn1; }
                    return;
                }
                if (x == 0) {
                    const double lo = hmq ? lpOffH : lpOffR;
                    p0 = (lo + lIns0) + pin0; p1 = (lo + lIns1) + pin0;
                } else {
                    int dd = pinD0 + x;
                    dd = dd < 0 ? -dd : dd;                              // Library::getProb (Library.hpp:60-64)
                    dd = dd >= pinMax ? pinMax - 1 : dd;
                    const double pin = (x >= 1 && x <= Hs) ? P.lib_logprob[pinBase + dd] : 0.0;
                    const double lo = hmq ? lpOnH : lpOnR;
                    p0 = (pin + lo) + lIns0; p1 = (pin + lo) + lIns1;
                }
            };
            // base[x] = alpha + obs + beta (:1098) for both state kinds; the two slices (read's mapping quality, then 1-1e-10) are formed one
            // after the other from it, so that alpha / beta and the first slice are dead while the second lives
            double bA[K], bI[K], vA[K], vI[K];
            double on = LNEG_INF;
#pragma unroll
            for (int k = 0; k < K; k++) {
                const int x = k * NT + t;
                const double o = ((sym_mask(sc[x]) >> col) & 1u) ? eq : uq;
                bA[k] = (a[k] + o) + (STASH ? beS[k * NT + t] : be_a[STASH ? 0 : k]);
                bI[k] = (in[k] + eq) + (STASH ? beS[NP + k * NT + t] : be_i[STASH ? 0 : k]);
                double p0, p1;
                priors(x, false, p0, p1);
                vA[k] = bA[k] + p0;
                vI[k] = bI[k] + p1;
                if (x >= 1 && x <= Hs) {                                 // (:1106-1107) plain max
                    on = vA[k] > on ? vA[k] : on;
                    on = vI[k] > on ? vI[k] : on;
                }
                if (x == 0) llOff = vA[k] > vI[k] ? vA[k] : vI[k];       // states 0 and numS (:1104-1105); thread 0
            }
            llOn = block_max(on, red);
            double *scan = reinterpret_cast<double *>(rowA);             // near-tie replay scratch (the row is free now)
            block_argmax<K>(vA, vI, numS, scan, red, redi, ll, mapRMQ);
#pragma unroll
            for (int k = 0; k < K; k++) {
                double p0, p1;
                priors(k * NT + t, true, p0, p1);
                vA[k] = bA[k] + p0;
                vI[k] = bI[k] + p1;
            }
            block_argmax<K>(vA, vI, numS, scan, red, redi, llHMQ, mapHMQ);
        }
        if (wave != 0) continue;                                         // wavefront 0 finishes the pair

        const int xR = mapRMQ % numS, xH = mapHMQ % numS;
        const bool offHap = (xR == 0 || xR == RO);
        const bool offHapHMQ = (xH == 0 || xH == RO);
        // ================= traceback: computeMAPState (:1148-1165), the main kernel's run detection (64 rows at a time)
        {
            auto fieldAt = [&](int row, int x) -> unsigned { return (unsigned)reinterpret_cast<const bt_t *>(tile)[(size_t)row * NP + x] & FMASK; };
            const int s0 = __builtin_amdgcn_readfirstlane(mapHMQ);
            if (lane == 0) ms[bMid] = (int16_t)s0;
            {   // towards base 0: mapState[b-1] = btf[b][mapState[b]]
                int ins = s0 >= numS ? 1 : 0, x = s0 - (ins ? numS : 0), b = bMid;
                while (b > 0) {
                    unsigned f;
                    if (!ins && x == 0) {                                 // LO is absorbing in this direction
                        for (int j = lane; j < b; j += 64) ms[j] = 0;
                        break;
                    }
                    if (!ins && x != RO) {                                // diagonal run
                        const int maxrun = b < 64 ? b : 64;
                        const bool valid = lane < maxrun && x - lane >= 1;
                        f = valid ? fieldAt(b - lane, x - lane) : 0u;
                        const unsigned long long m = __ballot(valid && (f & CHMASK) == 1u);
                        const int run = (m == ~0ull) ? 64 : __builtin_ctzll(~m);
                        if (lane < run) ms[b - 1 - lane] = (int16_t)(x - 1 - lane);
                        b -= run; x -= run;
                        if (b == 0) break;
                        if (run == maxrun || x == 0) continue;
                        f = (unsigned)__builtin_amdgcn_readlane((int)f, run);
                    } else {
                        f = (unsigned)__builtin_amdgcn_readfirstlane((int)fieldAt(b, x));
                    }
                    // on base x: ch = jump length y (from x-y), 0 = from numS+x-1; RO: 0 RO, 1 Hs, 2 numS+RO, 3 numS+Hs;
                    // inserted at x: bit set = entered from "on base x", else stays
                    const int ch = (int)(f & CHMASK), ib = (int)(f >> CB);
                    const int z = ch == 0 ? 1 : 0;
                    int gx = x - ch - z, gi = z;
                    if (x == RO) { gx = RO - (ch & 1); gi = ch >> 1; }
                    if (ins) { gx = x; gi = ib ^ 1; }
                    x = gx; ins = gi;
                    if (lane == 0) ms[b - 1] = (int16_t)(ins ? numS + x : x);
                    b--;
                }
            }
            {   // towards base L-1: mapState[b+1] = btb[b][mapState[b]], stored at row b+1
                int ins = s0 >= numS ? 1 : 0, x = s0 - (ins ? numS : 0), b = bMid;
                while (b < L - 1) {
                    unsigned f;
                    if (!ins) {
                        const int left = L - 1 - b, maxrun = left < 64 ? left : 64;
                        const bool stay = (x == 0 || x == RO);
                        const bool valid = lane < maxrun && (stay || x + lane <= Hs);
                        f = valid ? fieldAt(b + 1 + lane, stay ? x : x + lane) : 0u;
                        const unsigned long long m = __ballot(valid && (f & CHMASK) == (stay ? 0u : 1u));
                        const int run = (m == ~0ull) ? 64 : __builtin_ctzll(~m);
                        if (lane < run) ms[b + 1 + lane] = (int16_t)(stay ? x : x + 1 + lane);
                        b += run;
                        if (!stay) x += run;
                        if (b >= L - 1) break;
                        if (run == maxrun) continue;
                        if (!stay && x > Hs) continue;
                        f = (unsigned)__builtin_amdgcn_readlane((int)f, run);
                    } else {
                        f = (unsigned)__builtin_amdgcn_readfirstlane((int)fieldAt(b + 1, x));
                    }
                    // on base x: ch = jump length y (to x+y), 0 = to numS+x; LO: 0 LO, 1 base 1, 2 numS; RO: 0 RO, else numS+RO;
                    // inserted at x: bit set = leaves to min(x+1, RO) (LO's stays LO), else stays
                    const int ch = (int)(f & CHMASK), ib = (int)(f >> CB);
                    const int z = ch == 0 ? 1 : 0;
                    int gx = x + ch, gi = z;
                    if (x == RO) { gx = RO; gi = z ^ 1; }
                    if (x == 0) { gx = ch & 1; gi = ch >> 1; }
                    if (ins) {
                        int lx = x + 1 > RO ? RO : x + 1;
                        if (x == 0) lx = 0;
                        gx = ib ? lx : x;
                        gi = ib ^ 1;
                    }
                    x = gx; ins = gi;
                    if (lane == 0) ms[b + 1] = (int16_t)(ins ? numS + x : x);
                    b++;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        // ================= reportVariants (:1351-1475): hpos + QC counters, lane-parallel over read bases
        int nIndel = 0, nMis = 0, nBQT = 0, nmmBQT = 0, nMML = 0, nMMR = 0;
        int firstB = 0x7fffffff, lastB = -1;
        double mLogBQ = 0.0;
        const double thr = T[TC_BQT];
        const int rs_base = P.read_seq_off[r0];
        const int64_t SL = (int64_t)P.read_seq_off[r1] - rs_base;
        int16_t *hp_out = P.out.hpos ? P.out.hpos + P.win_hpos_off[w] + (int64_t)hi_ * SL + (so - rs_base) : nullptr;
        for (int b0 = 0; b0 < L; b0 += 64) {
            const int b = b0 + lane;
            double cb = 0.0;
            bool pIndel = false, pDel = false, pMis = false, pBQT = false, pmmBQT = false, pL = false, pR = false;
            if (b < L) {
                const int s = ms[b];
                const bool ins = s >= numS;
                const int x = ins ? s - numS : s;
                int hpv;
                if (x == 0) hpv = DD_HPOS_LO;
                else if (x == RO) hpv = DD_HPOS_RO;
                else if (ins) {
                    hpv = DD_HPOS_INS_KEY0 - x;                              // inserted base, carrying its key (pos = x, :1380)
                    pIndel = (b == 0 || ms[b - 1] < numS);                   // start of an insertion run (:1379-1394)
                } else {
                    hpv = x - 1;
                    firstB = hpv < firstB ? hpv : firstB;
                    lastB = hpv > lastB ? hpv : lastB;
                    const int qi = rdQ[b];
                    const double q = shQ[4 * qi + 3];
                    const bool hiq = q > thr;
                    if (hiq) { pBQT = true; cb = shQ[4 * qi + 2]; }          // (:1404-1407)
                    if ((int)rdC[b] != (int)sc[x]) {                         // read.seq[b]!=hap.seq[s-1] (:1410)
                        pmmBQT = hiq;
                        pL = b < 6;
                        pR = b > L - 6;
                        pMis = q > 0.95;
                    }
                    if (b < L - 1) {
                        const int ns = ms[b + 1];
                        pDel = (ns < numS && ns - s > 1);                    // deletion (:1437-1453)
                    }
                }
                if (hp_out) hp_out[b] = (int16_t)hpv;
            }
            nIndel += __popcll(__ballot(pIndel)) + __popcll(__ballot(pDel));
            nMis += __popcll(__ballot(pMis));
            nmmBQT += __popcll(__ballot(pmmBQT));
            nMML += __popcll(__ballot(pL));
            nMMR += __popcll(__ballot(pR));
            const unsigned long long bq = __ballot(pBQT);
            nBQT += __popcll(bq);
            // mLogBQ: log10(1-q) added base by base in read order (:1404-1407); +0.0 for the other bases is exact
            if (bq) {
                if (b < L) red[lane] = cb;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const int first = __ffsll((long long)bq) - 1, last = 63 - __clzll((long long)bq);
                for (int i = first; i <= last; i++) mLogBQ += red[i];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const int f = __shfl_xor(firstB, off), l2 = __shfl_xor(lastB, off);
            firstB = f < firstB ? f : firstB;
            lastB = l2 > lastB ? l2 : lastB;
        }
        if (firstB == 0x7fffffff) firstB = -1;

        // hapIndelCovered / hapSNPCovered (:1465-1472; AlignedVariant::isCovered Variant.hpp:125-128)
        if (P.out.var_covered && nv > 0) {
            for (int i = lane; i < nv; i += 64) {
                const int sR = P.hap_var[2 * (P.hap_var_off[g] + i)];
                const int eR = P.hap_var[2 * (P.hap_var_off[g] + i) + 1];
                P.out.var_covered[vb + i] = (firstB + P.padCover <= sR && lastB - P.padCover >= eR) ? 1 : 0;
            }
        }
        // filterHaplotypes' per-read coverage test of the haplotype's own indels (DInDel.cpp:1951-2062)
        if (P.out.var_fcov && P.hap_var_flank && nv > 0) {
            const bool sel = !offHapHMQ && nIndel == 0;
            for (int i = 0; i < nv; i++) {
                const int32_t *fl = P.hap_var_flank + 3 * (size_t)(P.hap_var_off[g] + i);
                const int left = fl[0] - P.padCover, right = fl[1] + P.padCover, kind = fl[2];
                int cov = 0;
                if (sel && kind != 0) {
                    int nmm = 0;
                    for (int b0 = 0; b0 < L; b0 += 64) {
                        const int b = b0 + lane;
                        bool mm = false;
                        if (b < L) {
                            const int s = ms[b];
                            if (s >= 1 && s <= Hs) {
                                const int hb = s - 1;
                                const int hcode = sc[s];
                                mm = hb >= left && hb <= right && (int)rdC[b] != hcode && (kind == 2 || hcode != SYM_N);   // 'N' exempt for DEL (:1992)
                            }
                        }
                        nmm += __popcll(__ballot(mm));
                    }
                    const int lo2 = firstB > left ? firstB : left, hi2 = lastB < right ? lastB : right;
                    const int csize = (firstB >= 0 && hi2 >= lo2) ? hi2 - lo2 + 1 : 0;
                    cov = (csize >= right - left + 1 && nmm <= P.maxMismatch) ? 1 : 0;
                }
                if (lane == 0) P.out.var_fcov[vb + i] = (uint8_t)cov;
            }
        }

        if (lane == 0) {
            int status = DD_PAIR_OK;
            if (ll > 0.1) status = DD_PAIR_LLPOS;                                // DInDel.cpp:1722
            else if (ll != ll || ll == LNEG_INF || ll == -LNEG_INF) status = DD_PAIR_NAN;   // DInDel.cpp:1732
            P.out.ll[pair] = ll;
            P.out.status[pair] = status;
            if (P.out.llOn) P.out.llOn[pair] = llOn;
            if (P.out.llOff) P.out.llOff[pair] = llOff;
            if (P.out.mLogBQ) P.out.mLogBQ[pair] = mLogBQ;
            if (P.out.offHap) P.out.offHap[pair] = offHap ? 1 : 0;
            if (P.out.offHapHMQ) P.out.offHapHMQ[pair] = offHapHMQ ? 1 : 0;
            if (P.out.numIndels) P.out.numIndels[pair] = (int16_t)nIndel;
            if (P.out.numMismatch) P.out.numMismatch[pair] = (int16_t)nMis;
            if (P.out.nBQT) P.out.nBQT[pair] = (int16_t)nBQT;
            if (P.out.nmmBQT) P.out.nmmBQT[pair] = (int16_t)nmmBQT;
            if (P.out.nMMLeft) P.out.nMMLeft[pair] = (int16_t)nMML;
            if (P.out.nMMRight) P.out.nMMRight[pair] = (int16_t)nMMR;
            if (P.out.firstBase) P.out.firstBase[pair] = (int16_t)firstB;
            if (P.out.lastBase) P.out.lastBase[pair] = (int16_t)lastB;
        }
    }
    if (t == 0 && my_pairs) {
        atomicAdd(&P.stats[0], my_pairs);
        atomicMax(&P.stats[1], my_pairs);
    }
}

// onHap[r] of the long windows' reads, after the long kernel (kernel_common.h)
__global__ void dd_long_onhap_kernel(const LongArgs P) { ddc::onhap_of_read(P); }

// A wide launch has no main launch in front of it: the pairs of the windows of [w_begin, w_end) that are not DD_WIN_LONG get here the
// placeholder the main kernels give a screened window (hmm_kernel.hip mark_unsupported).  One workgroup per window.
__global__ void __launch_bounds__(256) dd_wide_placeholder_kernel(const LongArgs P)
{
    const int w = P.w_begin + (int)blockIdx.x;
    if (w >= P.w_end || P.win_class[w] == DD_WIN_LONG) return;
    const int64_t p0 = P.win_pair_off[w], p1 = P.win_pair_off[w + 1];
    for (int64_t pair = p0 + threadIdx.x; pair < p1; pair += blockDim.x) {
        P.out.status[pair] = DD_PAIR_UNSUPPORTED;
        P.out.ll[pair] = 0.0;
        if (P.out.offHap) P.out.offHap[pair] = 1;
        if (P.out.offHapHMQ) P.out.offHapHMQ[pair] = 1;
    }
}

// ... and onHap[r] of every read of [read_begin, read_end), after the kernels above (a placeholder window's pairs are all
// DD_PAIR_UNSUPPORTED: its reads get 0, as from the main launch's pass)
__global__ void dd_wide_onhap_kernel(const LongArgs P) { ddc::onhap_of_read<true>(P); }

size_t long_lds_layout(int K, int max_read_len, LongArgs &A)
{
    const size_t NP = (size_t)NT * K;
    size_t o = 16 * (NP + 2 * PAD);                    // rowA
    A.lds_off_rowI = up16(o); o = A.lds_off_rowI + 8 * (NP + 1);
    A.lds_off_EN = up16(o); o = A.lds_off_EN + 16 * (HP_DEF + 1);
    A.lds_off_Q = up16(o); o = A.lds_off_Q + 8 * 4 * (size_t)(A.n_qual > 0 ? A.n_qual : 1);
    A.lds_off_red = up16(o); o = A.lds_off_red + 8 * 64 + 4 * 16;
    A.lds_off_sc = up16(o); o = A.lds_off_sc + NP;
    A.lds_off_hc = up16(o); o = A.lds_off_hc + NP + 2 * PAD;
    A.lds_off_lut = up16(o); o = A.lds_off_lut + 256;
    A.lds_off_ms = up16(o); o = A.lds_off_ms + 2 * (size_t)max_read_len;
    A.lds_off_rdC = up16(o); o = A.lds_off_rdC + (size_t)max_read_len;
    A.lds_off_rdQ = up16(o); o = A.lds_off_rdQ + (size_t)max_read_len;
    return up16(o);
}

template <int K, bool WIDE>
static hipError_t launch_k(const LongArgs &A, unsigned grid, size_t lds, hipStream_t st)
{
    // the dynamic-LDS cap is raised once per instance and device
    static std::atomic<unsigned> raised(0u);
    const hipError_t e = ddc::raise_lds_cap_once(reinterpret_cast<const void *>(&dd_long_kernel<K, WIDE>), raised);
    if (e != hipSuccess) return e;
    if (lds > 160u * 1024u) return hipErrorInvalidValue;
    hipLaunchKernelGGL((dd_long_kernel<K, WIDE>), dim3(grid), dim3(NT), lds, st, A);
    return hipGetLastError();
}

hipError_t launch_wide_tail(const LongArgs &A, bool onhap, hipStream_t st)
{
    hipError_t e = hipSuccess;
    if (A.w_end > A.w_begin) {
        hipLaunchKernelGGL(dd_wide_placeholder_kernel, dim3(A.w_end - A.w_begin), dim3(256), 0, st, A);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (onhap && A.read_end > A.read_begin) {
        hipLaunchKernelGGL(dd_wide_onhap_kernel, dim3((A.read_end - A.read_begin + 255) / 256), dim3(256), 0, st, A);
        e = hipGetLastError();
    }
    return e;
}

template <bool WIDE>
static hipError_t launch_build(int K, const LongArgs &A, unsigned grid, size_t lds, hipStream_t st)
{
    switch (K) {
    case 1: return launch_k<1, WIDE>(A, grid, lds, st);
    case 2: return launch_k<2, WIDE>(A, grid, lds, st);
    case 4: return launch_k<4, WIDE>(A, grid, lds, st);
    case 8: return launch_k<8, WIDE>(A, grid, lds, st);
    case 16: return launch_k<16, WIDE>(A, grid, lds, st);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_long(int K, bool wide, const LongArgs &A, unsigned grid, size_t lds, bool onhap, hipStream_t st)
{
    if (grid < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dd_long_prepass, dim3(1), dim3(1024), 0, st, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = wide ? launch_build<true>(K, A, grid, lds, st) : launch_build<false>(K, A, grid, lds, st);
    if (e != hipSuccess) return e;
    if (wide) return launch_wide_tail(A, onhap, st);
    if (onhap && A.read_end > A.read_begin) {
        hipLaunchKernelGGL(dd_long_onhap_kernel, dim3((A.read_end - A.read_begin + 255) / 256), dim3(256), 0, st, A);
        e = hipGetLastError();
    }
    return e;
}

} // namespace ddl
