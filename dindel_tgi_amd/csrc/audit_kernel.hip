// audit_kernel.hip — the comparison of an audit on the device: what the main kernels left for the audited pairs against the long-window
// kernel's shadow of them, bit for bit.  audit_kernel.h is the definition (au_compared, au_load, au_locate), shared with the CPU
// evaluation.
//
// One wavefront per audited pair, a persistent grid striding over the pairs (indel_keys_kernel.hip's mapping); no counter to draw from.
// Every lane loads the two statuses (one address: a broadcast).  Lane f < 15 then holds per-pair field f: lane 0 the status, lanes 1 ... 14
// the values the status opens.  The lanes run together over the pair's hpos entries and coverage bytes, 64 at a time.  Integer compares
// only, no LDS, no floating point: a double is loaded as its 64 bits.  The primary and the shadow are only read.
//
// The report: a lane that finds a difference draws a record slot with an ordinary atomic add on n_diff and, if the slot lies below
// max_records, writes the record with vector stores; the counts per field are summed in registers over the wavefront's pairs, reduced
// across the lanes once at the end, and added by one lane with one atomic per non-zero count.  Every loop is bounded by the pair's own
// lengths; no store goes anywhere but the report.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "audit_kernel.h"

namespace dda {
namespace {

__device__ __forceinline__ void add64(int64_t *at, long long v)
{
    if (v) atomicAdd(reinterpret_cast<unsigned long long *>(at), (unsigned long long)v);
}

__device__ __forceinline__ long long wave_sum(long long v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ void record(const AuditArgs &P, int w, int field, int64_t pair, int64_t index, uint64_t a, uint64_t b)
{
    const unsigned long long slot = atomicAdd(reinterpret_cast<unsigned long long *>(&P.report->n_diff), 1ull);
    if ((int64_t)slot < P.max_records) {
        dd_audit_record &r = P.records[slot];
        r.window = w; r.field = field; r.pair = pair; r.index = index; r.primary_bits = a; r.shadow_bits = b;
    }
}

// the elements [0, n) of a per-element field of one pair, 64 at a time; -> this lane's differences
__device__ __forceinline__ int compare_run(const AuditArgs &P, const au_pair &a, int field, int size, int64_t p0, int64_t s0, int n, int lane)
{
    const void *pa = P.primary.f[field], *sa = P.shadow.f[field];
    int diff = 0;
    for (int i = lane; i < n; i += 64) {
        const uint64_t x = au_load(pa, p0 + i, size), y = au_load(sa, s0 + i, size);
        if (x != y) { diff++; record(P, a.w, field, a.p_pair, p0 + i, x, y); }
    }
    return diff;
}

} // namespace

__global__ void __launch_bounds__(64 * DD_AUDIT_WAVES) dd_audit_compare_kernel(AuditArgs P)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t stride = (int64_t)gridDim.x * DD_AUDIT_WAVES;
    // lane f < 15: elements compared / differences of per-pair field f; every lane: its share of the three per-element fields
    long long cmp_pair = 0, diff_pair = 0, cmp_h = 0, diff_h = 0, cmp_c = 0, diff_c = 0, cmp_f = 0, diff_f = 0, n_pairs = 0;
    const int my_field = lane < DD_AUDIT_N_PAIR_FIELDS ? lane : 0;
    const void *my_p = P.primary.f[my_field], *my_s = P.shadow.f[my_field];
    const bool mine = lane < DD_AUDIT_N_PAIR_FIELDS && my_p && my_s;
    const int my_size = au_field_size(my_field);
    const bool have_h = P.primary.f[DD_AUDIT_FIELD_hpos] && P.shadow.f[DD_AUDIT_FIELD_hpos];
    const bool have_c = P.primary.f[DD_AUDIT_FIELD_var_covered] && P.shadow.f[DD_AUDIT_FIELD_var_covered];
    const bool have_f = P.primary.f[DD_AUDIT_FIELD_var_fcov] && P.shadow.f[DD_AUDIT_FIELD_var_fcov];

    for (int64_t j = P.j_begin + (int64_t)blockIdx.x * DD_AUDIT_WAVES + wave; j < P.j_end; j += stride) {
        const au_pair a = au_locate(&P.G, j);                   // wave-uniform
        const int st_p = (int)au_load(P.primary.f[DD_AUDIT_FIELD_status], a.p_pair, 4);
        const int st_s = (int)au_load(P.shadow.f[DD_AUDIT_FIELD_status], a.s_pair, 4);
        n_pairs++;
        const uint32_t open = st_p == st_s ? au_compared(st_p, P.has_flank) : 1u << DD_AUDIT_FIELD_status;
        if (mine && (open >> lane & 1u)) {
            const uint64_t x = au_load(my_p, a.p_pair, my_size), y = au_load(my_s, a.s_pair, my_size);
            cmp_pair++;
            if (x != y) { diff_pair++; record(P, a.w, lane, a.p_pair, a.p_pair, x, y); }
        }
        if (have_h && (open >> DD_AUDIT_FIELD_hpos & 1u)) {
            diff_h += compare_run(P, a, DD_AUDIT_FIELD_hpos, 2, a.p_hpos, a.s_hpos, a.L, lane);
            if (lane == 0) cmp_h += a.L;
        }
        if (have_c && (open >> DD_AUDIT_FIELD_var_covered & 1u)) {
            diff_c += compare_run(P, a, DD_AUDIT_FIELD_var_covered, 1, a.p_cov, a.s_cov, a.nv, lane);
            if (lane == 0) cmp_c += a.nv;
        }
        if (have_f && (open >> DD_AUDIT_FIELD_var_fcov & 1u)) {
            diff_f += compare_run(P, a, DD_AUDIT_FIELD_var_fcov, 1, a.p_cov, a.s_cov, a.nv, lane);
            if (lane == 0) cmp_f += a.nv;
        }
    }

    // the wavefront's counts into the report: lanes 0 ... 14 their own field's, lane 0 the reduced rest
    if (lane < DD_AUDIT_N_PAIR_FIELDS) { add64(&P.report->compared[lane], cmp_pair); add64(&P.report->diff[lane], diff_pair); }
    diff_h = wave_sum(diff_h); diff_c = wave_sum(diff_c); diff_f = wave_sum(diff_f);
    if (lane == 0) {
        add64(&P.report->n_pairs, n_pairs);
        add64(&P.report->compared[DD_AUDIT_FIELD_hpos], cmp_h); add64(&P.report->diff[DD_AUDIT_FIELD_hpos], diff_h);
        add64(&P.report->compared[DD_AUDIT_FIELD_var_covered], cmp_c); add64(&P.report->diff[DD_AUDIT_FIELD_var_covered], diff_c);
        add64(&P.report->compared[DD_AUDIT_FIELD_var_fcov], cmp_f); add64(&P.report->diff[DD_AUDIT_FIELD_var_fcov], diff_f);
    }
}

unsigned audit_grid(int64_t n_pairs)
{
    if (n_pairs <= 0) return 0;
    int64_t blocks = (n_pairs + DD_AUDIT_WAVES - 1) / DD_AUDIT_WAVES;
    if (blocks > DD_AUDIT_MAX_BLOCKS) blocks = DD_AUDIT_MAX_BLOCKS;
    return (unsigned)blocks;
}

hipError_t launch_audit_compare(const AuditArgs &A, hipStream_t st)
{
    const unsigned blocks = audit_grid(A.j_end - A.j_begin);
    if (!blocks) return hipSuccess;
    hipLaunchKernelGGL(dd_audit_compare_kernel, dim3(blocks), dim3(64 * DD_AUDIT_WAVES), 0, st, A);
    return hipGetLastError();
}

} // namespace dda
