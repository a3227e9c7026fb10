// faster_shadow_kernel.hip — the shadow of an audit of the --faster model (include/dindel_hmm.h, "audit of the --faster model"): the pairs
// of a sample recomputed with faster_shadow.h's functions, and the comparison of a --faster launch's results with that shadow under
// au_compared_faster.  The model is the header's; this file only deals it out over a wavefront.  It includes nothing of the two --faster
// kernels (their model header and its two fragments) and is laid out unlike them: they put four pairs on 16-lane groups, lane = diagonal.
//
// dd_faster_shadow_kernel: one wavefront per audited pair, a persistent grid of at most DD_FS_MAX_BLOCKS workgroups of DD_FS_WAVES
// wavefronts striding over the sample's pairs; the pair's window by bisection in the sample's pair offsets (fs_locate).
//   votes       lanes stride over the haplotype's positions; counts go into a wave-private integer histogram with ordinary atomics, so
//               the result does not depend on the order of arrival
//   top 15      fifteen wave-wide (highest count, lowest bin) reductions; one lane appends the sentinel and sorts
//   sweeps      lane t < 2S owns destination state t and calls fs_left_step / fs_right_step; the two alpha rows ping-pong in wave-private
//               LDS, one back-pointer byte per state and base goes to the wavefront's tile
//   join        a wave reduction that keeps the lowest state among equal maxima
//   traceback, mapState   serial on one lane
//   hpos, coverage bytes, per-pair values   vector stores spread over the lanes
// A wavefront's area (back-pointer tile, over the dead vote histogram; state path, over the dead read keys; mapState) is in LDS while the
// sample's longest haplotype and read are ordinary (<= DD_MAX_HAP_LEN, DD_MAX_READ_LEN), else in an HBM workspace sized by the grid.
// Lanes of one wavefront hand data to each other through that area: lanes_sync() is a release fence, a wave barrier and an acquire fence.
// Every loop is bounded by the pair's own lengths, which are checked against what the areas were sized for; stores go to the shadow, the
// area and the report only.  No inline assembly, no scratch.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <stdint.h>
#include "kernel_common.h"
#include "faster_shadow.h"

namespace dfs {
namespace {

constexpr uint32_t kSmallRel = 0, kSmallRows = 64, kSmallBits = kSmallRows + 2 * FS_MAX_STATES * 8, kSmallBytes = kSmallBits + FS_COV_WORDS * 4;
static_assert(kSmallBytes % 16 == 0 && (FS_MAX_DIAGONALS + 1) * 4 <= kSmallRows, "the wave-private fixed part");

struct AreaLayout { uint32_t off_path, off_ms, bytes; };
inline AreaLayout area_layout(int max_hap_len, int max_read_len)
{
    const size_t L = (size_t)max_read_len, H = (size_t)max_hap_len;
    AreaLayout a;
    a.off_path = ddc::up16(std::max(L * FS_MAX_STATES, (L + H) * 4));
    a.off_ms = a.off_path + ddc::up16(L);
    a.bytes = a.off_ms + ddc::up16(2 * L);
    return a;
}

__device__ __forceinline__ void lanes_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(v, off); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ int wave_add(int v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ int wave_min(int v)
{
    for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(v, off); v = o < v ? o : v; }
    return v;
}

// the fields the model leaves at MLAlignment's defaults, one lane each (field ids 2 ... 12)
__device__ __forceinline__ void store_defaults(const dd_result &o, int64_t at, int lane, bool computed)
{
    if (lane == DD_AUDIT_FIELD_llOn && o.llOn) o.llOn[at] = 0.0;
    if (lane == DD_AUDIT_FIELD_llOff && o.llOff) o.llOff[at] = 0.0;
    if (lane == DD_AUDIT_FIELD_mLogBQ && o.mLogBQ) o.mLogBQ[at] = 0.0;
    if (lane == DD_AUDIT_FIELD_offHap && o.offHap) o.offHap[at] = 0;
    if (lane == DD_AUDIT_FIELD_offHapHMQ && o.offHapHMQ) o.offHapHMQ[at] = computed ? 0 : 1;
    if (lane == DD_AUDIT_FIELD_numIndels && o.numIndels) o.numIndels[at] = 0;
    if (lane == DD_AUDIT_FIELD_numMismatch && o.numMismatch) o.numMismatch[at] = 0;
    if (lane == DD_AUDIT_FIELD_nBQT && o.nBQT) o.nBQT[at] = 0;
    if (lane == DD_AUDIT_FIELD_nmmBQT && o.nmmBQT) o.nmmBQT[at] = 0;
    if (lane == DD_AUDIT_FIELD_nMMLeft && o.nMMLeft) o.nMMLeft[at] = 0;
    if (lane == DD_AUDIT_FIELD_nMMRight && o.nMMRight) o.nMMRight[at] = 0;
}

} // namespace

__global__ void __launch_bounds__(64 * DD_FS_WAVES) dd_faster_shadow_kernel(const ShadowArgs P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    unsigned char *fixed = smem + (size_t)wave * kSmallBytes;
    int32_t *rel = reinterpret_cast<int32_t *>(fixed + kSmallRel);
    double *rows = reinterpret_cast<double *>(fixed + kSmallRows);
    uint32_t *bits = reinterpret_cast<uint32_t *>(fixed + kSmallBits);
    unsigned char *area = P.ws ? P.ws + ((size_t)blockIdx.x * DD_FS_WAVES + wave) * P.area_bytes
                               : smem + DD_FS_WAVES * kSmallBytes + (size_t)wave * P.area_bytes;
    int32_t *hist = reinterpret_cast<int32_t *>(area);               // dead once the diagonals are chosen
    uint8_t *bt = area;                                              // ... and then the back-pointer tile
    uint8_t *rk = area + P.off_path;                                 // the read's 4-mer keys: dead once the votes are cast
    uint8_t *path = area + P.off_path;                               // ... and then the state path
    int16_t *ms = reinterpret_cast<int16_t *>(area + P.off_ms);
    const dd_result &o = P.out;
    const int64_t stride = (int64_t)gridDim.x * DD_FS_WAVES;

    for (int64_t j = P.j_begin + (int64_t)blockIdx.x * DD_FS_WAVES + wave; j < P.j_end; j += stride) {
        const fs_where x = fs_locate(&P.G, j);                       // wave-uniform, as everything derived from it
        const au_pair &a = x.a;
        const int hs = P.hap_seq_off[x.g], hlen = P.hap_seq_off[x.g + 1] - hs, L = a.L;
        const int64_t so = (int64_t)P.G.read_seq_off[x.q];
        if (hlen < 0 || L < 0 || hlen > P.max_hap_len || L > P.max_read_len) continue;      // not what the areas were sized for: not computed
        const int v0 = a.nv > 0 ? P.G.hap_var_off[x.g] : 0;
        const int status = fs_status(P.maxLengthDel, hlen, L);
        store_defaults(o, a.s_pair, lane, status == DD_PAIR_OK);
        if (status != DD_PAIR_OK) {
            if (lane == 0) o.status[a.s_pair] = status;
            if (lane == 1) o.ll[a.s_pair] = 0.0;
            for (int i = lane; i < a.nv; i += 64) {
                if (o.var_covered) o.var_covered[a.s_cov + i] = 0;
                if (o.var_fcov) o.var_fcov[a.s_cov + i] = 0;
            }
            continue;
        }
        fs_pair pr;
        pr.hap = P.hap_seq + hs; pr.read = P.read_seq + so; pr.qidx = P.read_qidx + so; pr.T = P.tables; pr.rel = rel;
        pr.hlen = hlen; pr.L = L; pr.mqidx = P.read_mqidx[x.q];
        pr.bMid = fs_bmid(P.win_hap_start[a.w], hlen, P.read_start[x.q], L);

        // ---- votes ----
        lanes_sync();                                                // the previous pair's readers of the area are done
        const int nbins = fs_n_bins(hlen, L);
        for (int i = lane; i < nbins; i += 64) hist[i] = 0;
        for (int k = lane; k < fs_n_read_kmers(L); k += 64) rk[k] = (uint8_t)fs_kmer_key(pr.read, k);
        lanes_sync();
        for (int hx = lane; hx < fs_n_hap_kmers(hlen); hx += 64) fs_vote_hap_pos(pr.hap, hx, rk, L, hist);
        lanes_sync();
        // ---- the diagonals ----
        int n = 0;
        for (int round = 0; round < FS_MAX_DIAGONALS; round++) {
            unsigned long long best = 0;
            for (int i = lane; i < nbins; i += 64) {
                const unsigned long long k = fs_vote_rank(hist[i], i);
                best = k > best ? k : best;
            }
            best = wave_max(best);
            if (!best) break;
            const int bin = fs_rank_bin(best);
            if (lane == 0) { rel[n] = bin - L; hist[bin] = 0; }
            n++;
            lanes_sync();
        }
        if (lane == 0) (void)fs_sort_diagonals(rel, n, L);
        pr.S = n + 1;
        lanes_sync();

        // ---- the two sweeps towards bMid: lane t owns destination state t ----
        const bool mine = lane < 2 * pr.S;
        double leftv = 0.0, rightv = 0.0;
        for (int r = 0; r < pr.bMid; r++) {
            if (mine) {
                const fs_cell c = fs_left_step(&pr, lane, r, rows + ((r + 1) & 1) * FS_MAX_STATES);
                rows[(r & 1) * FS_MAX_STATES + lane] = c.v;
                bt[(size_t)r * FS_MAX_STATES + lane] = (uint8_t)c.bp;
                leftv = c.v;
            }
            lanes_sync();
        }
        for (int r = L - 1; r > pr.bMid; r--) {
            if (mine) {
                const fs_cell c = fs_right_step(&pr, lane, r, rows + ((r + 1) & 1) * FS_MAX_STATES);
                rows[(r & 1) * FS_MAX_STATES + lane] = c.v;
                bt[(size_t)r * FS_MAX_STATES + lane] = (uint8_t)c.bp;
                rightv = c.v;
            }
            lanes_sync();
        }
        // ---- the join: the maximum for ll; for the path the first maximum in state order under the fixed mapping quality ----
        const double ninf = -__builtin_huge_val();
        double v = ninf, h = ninf;
        int xh = 64;
        if (mine) { v = fs_join(&pr, lane, 0, leftv, rightv); h = fs_join(&pr, lane, 1, leftv, rightv); xh = lane; }
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(v, off), oh = __shfl_xor(h, off);
            const int ox = __shfl_xor(xh, off);
            v = ov > v ? ov : v;
            const bool take = oh > h || (oh == h && ox < xh);
            h = take ? oh : h;
            xh = take ? ox : xh;
        }
        const int xmax = (h > ninf) ? xh : 0;                        // nothing above minus infinity: the reference's xmax stays 0
        if (lane == 0) fs_traceback(&pr, bt, xmax, path, ms);
        lanes_sync();

        // ---- hpos, firstBase / lastBase ----
        int firstB = 0x7fffffff, lastB = -1;
        for (int b = lane; b < L; b += 64) {
            int hb;
            const int hp = fs_hpos_of(ms[b], hlen, &hb);
            if (o.hpos) o.hpos[a.s_hpos + b] = (int16_t)hp;
            if (hb >= 0) { firstB = hb < firstB ? hb : firstB; lastB = hb > lastB ? hb : lastB; }
        }
        firstB = wave_min(firstB);
        lastB = -wave_min(-lastB);
        if (firstB == 0x7fffffff) firstB = -1;
        // ---- coverage ----
        if (o.var_covered)
            for (int i = lane; i < a.nv; i += 64)
                o.var_covered[a.s_cov + i] = (uint8_t)fs_var_covered(firstB, lastB, P.padCover, P.hap_var[2 * (v0 + i)], P.hap_var[2 * (v0 + i) + 1]);
        if (o.var_fcov && P.hap_var_flank)
            for (int i = 0; i < a.nv; i++) {
                const int32_t *fl = P.hap_var_flank + 3 * (size_t)(v0 + i);
                const int lo = fl[0] - P.padCover, hi = fl[1] + P.padCover, kind = fl[2];
                int cov = 0;
                if (kind != 0 && hi >= lo) {
                    for (int k = lane; k < FS_COV_WORDS; k += 64) bits[k] = 0;
                    lanes_sync();
                    int nmm = 0, marked = 0;
                    for (int b = lane; b < L; b += 64) nmm += fs_fcov_base(&pr, ms, b, lo, hi, kind, bits);
                    lanes_sync();
                    const int y1 = hi < hlen - 1 ? hi : hlen - 1;
                    for (int y = (lo > 0 ? lo : 0) + lane; y <= y1; y += 64) marked += fs_fcov_bit(bits, y);
                    nmm = wave_add(nmm);
                    marked = wave_add(marked);
                    cov = marked >= hi - lo + 1 && nmm <= P.maxMismatch;
                    lanes_sync();                                    // the bitmap's readers are done before the next variant clears it
                }
                if (lane == 0) o.var_fcov[a.s_cov + i] = (uint8_t)cov;
            }
        // ---- the pair's values ----
        if (lane == 0) o.status[a.s_pair] = DD_PAIR_OK;
        if (lane == 1) o.ll[a.s_pair] = v;
        if (lane == DD_AUDIT_FIELD_firstBase && o.firstBase) o.firstBase[a.s_pair] = (int16_t)firstB;
        if (lane == DD_AUDIT_FIELD_lastBase && o.lastBase) o.lastBase[a.s_pair] = (int16_t)lastB;
    }
}

// ---- the comparison under au_compared_faster: audit_kernel.hip's geometry (one wavefront per pair, lane f < 15 holds per-pair field f, the
// lanes run together over hpos and the coverage bytes), a kernel of its own so that the main model's comparison stays as it is ----
namespace {
__device__ __forceinline__ void add_count(int64_t *at, long long v)
{
    if (v) atomicAdd(reinterpret_cast<unsigned long long *>(at), (unsigned long long)v);
}
__device__ __forceinline__ long long wave_add64(long long v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ void note_difference(const dda::AuditArgs &P, int w, int field, int64_t pair, int64_t index, uint64_t x, uint64_t y)
{
    const unsigned long long slot = atomicAdd(reinterpret_cast<unsigned long long *>(&P.report->n_diff), 1ull);
    if ((int64_t)slot < P.max_records) {
        dd_audit_record &r = P.records[slot];
        r.window = w; r.field = field; r.pair = pair; r.index = index; r.primary_bits = x; r.shadow_bits = y;
    }
}
} // namespace

__global__ void __launch_bounds__(64 * DD_FS_WAVES) dd_audit_compare_faster_kernel(const dda::AuditArgs P)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t stride = (int64_t)gridDim.x * DD_FS_WAVES;
    const int pf = lane < DD_AUDIT_N_PAIR_FIELDS ? lane : 0;
    const bool have_pf = lane < DD_AUDIT_N_PAIR_FIELDS && P.primary.f[pf] && P.shadow.f[pf];
    const int run_field[3] = {DD_AUDIT_FIELD_hpos, DD_AUDIT_FIELD_var_covered, DD_AUDIT_FIELD_var_fcov};
    long long cmp_pf = 0, diff_pf = 0, n_pairs = 0;
    long long cmp_run0 = 0, cmp_run1 = 0, cmp_run2 = 0, diff_run0 = 0, diff_run1 = 0, diff_run2 = 0;

    for (int64_t j = P.j_begin + (int64_t)blockIdx.x * DD_FS_WAVES + wave; j < P.j_end; j += stride) {
        const au_pair a = au_locate(&P.G, j);
        const int st_p = (int)au_load(P.primary.f[DD_AUDIT_FIELD_status], a.p_pair, 4);
        const int st_s = (int)au_load(P.shadow.f[DD_AUDIT_FIELD_status], a.s_pair, 4);
        const uint32_t open = st_p == st_s ? au_compared_faster(st_p, P.has_flank) : 1u << DD_AUDIT_FIELD_status;
        n_pairs++;
        if (have_pf && (open >> lane & 1u)) {
            const int size = au_field_size(pf);
            const uint64_t xv = au_load(P.primary.f[pf], a.p_pair, size), yv = au_load(P.shadow.f[pf], a.s_pair, size);
            cmp_pf++;
            if (xv != yv) { diff_pf++; note_difference(P, a.w, pf, a.p_pair, a.p_pair, xv, yv); }
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int f = run_field[k];
            if (!(open >> f & 1u) || !P.primary.f[f] || !P.shadow.f[f]) continue;
            const int n = k == 0 ? a.L : a.nv, size = au_field_size(f);
            const int64_t p0 = k == 0 ? a.p_hpos : a.p_cov, s0 = k == 0 ? a.s_hpos : a.s_cov;
            int d = 0;
            for (int i = lane; i < n; i += 64) {
                const uint64_t xv = au_load(P.primary.f[f], p0 + i, size), yv = au_load(P.shadow.f[f], s0 + i, size);
                if (xv != yv) { d++; note_difference(P, a.w, f, a.p_pair, p0 + i, xv, yv); }
            }
            if (k == 0) { diff_run0 += d; cmp_run0 += lane == 0 ? n : 0; }
            if (k == 1) { diff_run1 += d; cmp_run1 += lane == 0 ? n : 0; }
            if (k == 2) { diff_run2 += d; cmp_run2 += lane == 0 ? n : 0; }
        }
    }
    if (lane < DD_AUDIT_N_PAIR_FIELDS) { add_count(&P.report->compared[lane], cmp_pf); add_count(&P.report->diff[lane], diff_pf); }
    diff_run0 = wave_add64(diff_run0); diff_run1 = wave_add64(diff_run1); diff_run2 = wave_add64(diff_run2);
    if (lane == 0) {
        add_count(&P.report->n_pairs, n_pairs);
        add_count(&P.report->compared[DD_AUDIT_FIELD_hpos], cmp_run0); add_count(&P.report->diff[DD_AUDIT_FIELD_hpos], diff_run0);
        add_count(&P.report->compared[DD_AUDIT_FIELD_var_covered], cmp_run1); add_count(&P.report->diff[DD_AUDIT_FIELD_var_covered], diff_run1);
        add_count(&P.report->compared[DD_AUDIT_FIELD_var_fcov], cmp_run2); add_count(&P.report->diff[DD_AUDIT_FIELD_var_fcov], diff_run2);
    }
}

// ---- host side of the unit ----
uint32_t area_bytes(int max_hap_len, int max_read_len) { return area_layout(max_hap_len, max_read_len).bytes; }
bool area_in_lds(int max_hap_len, int max_read_len) { return max_hap_len <= DD_MAX_HAP_LEN && max_read_len <= DD_MAX_READ_LEN; }
size_t shadow_lds_bytes(int max_hap_len, int max_read_len)
{
    return (size_t)DD_FS_WAVES * (kSmallBytes + (area_in_lds(max_hap_len, max_read_len) ? area_bytes(max_hap_len, max_read_len) : 0u));
}
unsigned shadow_grid(int64_t n_pairs, int max_hap_len, int max_read_len)
{
    if (n_pairs <= 0) return 0;
    int64_t blocks = (n_pairs + DD_FS_WAVES - 1) / DD_FS_WAVES;
    if (blocks > DD_FS_MAX_BLOCKS) blocks = DD_FS_MAX_BLOCKS;
    if (!area_in_lds(max_hap_len, max_read_len)) {
        const int64_t fit = (int64_t)(DD_FS_WS_BUDGET / ((size_t)DD_FS_WAVES * area_bytes(max_hap_len, max_read_len)));
        blocks = std::min(blocks, std::max<int64_t>(fit, 1));
    }
    return (unsigned)blocks;
}

hipError_t launch_shadow(const ShadowArgs &A0, hipStream_t st)
{
    const unsigned blocks = shadow_grid(A0.j_end - A0.j_begin, A0.max_hap_len, A0.max_read_len);
    if (!blocks) return hipSuccess;
    ShadowArgs A = A0;
    const AreaLayout lay = area_layout(A.max_hap_len, A.max_read_len);
    A.area_bytes = lay.bytes; A.off_path = lay.off_path; A.off_ms = lay.off_ms;
    const bool in_lds = area_in_lds(A.max_hap_len, A.max_read_len);
    if (in_lds) A.ws = nullptr;
    else if (!A.ws) return hipErrorInvalidValue;
    const size_t lds = shadow_lds_bytes(A.max_hap_len, A.max_read_len);
    if (lds > 160u * 1024u) return hipErrorInvalidValue;
    static std::atomic<unsigned> raised(0u);
    const hipError_t e = ddc::raise_lds_cap_once(reinterpret_cast<const void *>(&dd_faster_shadow_kernel), raised);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dd_faster_shadow_kernel, dim3(blocks), dim3(64 * DD_FS_WAVES), lds, st, A);
    return hipGetLastError();
}

hipError_t launch_compare_faster(const dda::AuditArgs &A, hipStream_t st)
{
    int64_t blocks = (A.j_end - A.j_begin + DD_FS_WAVES - 1) / DD_FS_WAVES;
    if (blocks <= 0) return hipSuccess;
    if (blocks > DD_FS_MAX_BLOCKS) blocks = DD_FS_MAX_BLOCKS;
    hipLaunchKernelGGL(dd_audit_compare_faster_kernel, dim3((unsigned)blocks), dim3(64 * DD_FS_WAVES), 0, st, A);
    return hipGetLastError();
}

} // namespace dfs
