/* audit_kernel.h — what an audit compares: the results the main kernels left for a pair against the long-window kernel's results for the
 * same pair (include/dindel_hmm.h, "audit").
 *
 * The first part of this file is plain C99 and is the definition: the kernel (audit_kernel.hip) and the CPU evaluation (audit_host.cpp,
 * dd_audit_compare_host) both ask au_compared() which fields a pair's status opens and read an element with au_load(), so the two cannot
 * drift apart.  The rule restates which elements of dd_result BOTH implementations of the main model are contracted to write for a pair
 * of a window they compute (dd_result and DD_PAIR_* in include/dindel_hmm.h; hmm_kernel.hip's and long_kernel.hip's stores):
 *
 *     status            always; if primary and shadow differ: one difference, and nothing else of the pair is compared (what the
 *                       other fields hold depends on the status, so every one of them would only repeat the finding)
 *     DD_PAIR_OK, DD_PAIR_NAN, DD_PAIR_LLPOS
 *                       the status is found from the finished ll, so everything is there: the 14 per-pair values ll, llOn, llOff, mLogBQ,
 *                       offHap, offHapHMQ, numIndels, numMismatch, nBQT, nmmBQT, nMMLeft, nMMRight, firstBase, lastBase; the pair's L
 *                       entries of hpos; its var_covered bytes; its var_fcov bytes when the batch has hap_var_flank
 *     DD_PAIR_HAPSIZE   "hapSize error.": ll (0) and the coverage flags (0), var_fcov again only with hap_var_flank; nothing else is written
 *     any other value   nothing more (DD_PAIR_UNSUPPORTED does not occur in a window both kernels compute)
 *     onHap             derived from offHapHMQ per read: never compared
 *
 * A field whose pointer is NULL on either side is skipped.  Equality is equality of bits: every element is loaded as an unsigned integer
 * of its width and zero-extended, so NaNs compare by payload and -0.0 differs from 0.0.  An element outside the rule is never read: the
 * primary and the shadow may hold different garbage there.
 *
 * Where a pair's elements lie: window w, haplotype h (of H), read r (of R), local = h R + r.
 *     per-pair values   primary: win_pair_off[w] + local                                  shadow: pair_off[w] + local
 *     hpos              primary: win_hpos_off[w] + h SL + (read_seq_off[q] - read_seq_off[q0]), L entries (SL: the window's read bases)
 *     coverage bytes    primary: win_varcov_off[w] + (hap_var_off[g] - hap_var_off[g0]) R + r nv, nv entries (nv: the haplotype's variants)
 *   and the shadow's likewise from the sample's own offsets (dd_audit_select): the layouts are the same, the origins differ.
 */
#ifndef DD_AUDIT_KERNEL_H
#define DD_AUDIT_KERNEL_H
#include <stdint.h>
#include <string.h>
#include "../../include/dindel_hmm.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define AU_FN static __host__ __device__ __forceinline__
#else
#define AU_FN static inline
#endif

#define DD_AUDIT_N_PAIR_FIELDS 15      /* status and the 14 per-pair values: field ids 0 ... 14 */

/* bytes of one element of field f */
AU_FN int au_field_size(int f)
{
    if (f == DD_AUDIT_FIELD_status) return 4;
    if (f >= DD_AUDIT_FIELD_ll && f <= DD_AUDIT_FIELD_mLogBQ) return 8;
    if (f == DD_AUDIT_FIELD_offHap || f == DD_AUDIT_FIELD_offHapHMQ || f == DD_AUDIT_FIELD_var_covered || f == DD_AUDIT_FIELD_var_fcov) return 1;
    return 2;
}

/* element i of an array of `size`-byte elements, zero-extended */
AU_FN uint64_t au_load(const void *base, int64_t i, int size)
{
    const unsigned char *at = (const unsigned char *)base + i * size;
    if (size == 8) { uint64_t v; memcpy(&v, __builtin_assume_aligned(at, 8), 8); return v; }   /* (memcpy: a double is read as its bits) */
    if (size == 4) { uint32_t v; memcpy(&v, __builtin_assume_aligned(at, 4), 4); return v; }
    if (size == 2) { uint16_t v; memcpy(&v, __builtin_assume_aligned(at, 2), 2); return v; }
    return *at;
}

/* The fields compared for a pair whose two statuses are both `status`, as a mask of 1 << DD_AUDIT_FIELD_*; status itself is always in it.
 * has_flank: the batch has hap_var_flank. */
AU_FN uint32_t au_compared(int status, int has_flank)
{
    const uint32_t st = 1u << DD_AUDIT_FIELD_status;
    const uint32_t cov = (1u << DD_AUDIT_FIELD_var_covered) | (has_flank ? 1u << DD_AUDIT_FIELD_var_fcov : 0u);
    if (status == DD_PAIR_OK || status == DD_PAIR_NAN || status == DD_PAIR_LLPOS)
        return (((1u << DD_AUDIT_N_PAIR_FIELDS) - 1u) | (1u << DD_AUDIT_FIELD_hpos) | cov);
    if (status == DD_PAIR_HAPSIZE) return st | (1u << DD_AUDIT_FIELD_ll) | cov;
    return st;
}

/* The two result blocks as arrays of untyped pointers, indexed by field id (C has no way to index a struct's members). */
typedef struct au_fields { const void *f[DD_AUDIT_N_FIELDS]; } au_fields;
AU_FN au_fields au_fields_of(const dd_result *r)
{
    au_fields a;
    a.f[DD_AUDIT_FIELD_status] = r->status; a.f[DD_AUDIT_FIELD_ll] = r->ll; a.f[DD_AUDIT_FIELD_llOn] = r->llOn; a.f[DD_AUDIT_FIELD_llOff] = r->llOff;
    a.f[DD_AUDIT_FIELD_mLogBQ] = r->mLogBQ; a.f[DD_AUDIT_FIELD_offHap] = r->offHap; a.f[DD_AUDIT_FIELD_offHapHMQ] = r->offHapHMQ;
    a.f[DD_AUDIT_FIELD_numIndels] = r->numIndels; a.f[DD_AUDIT_FIELD_numMismatch] = r->numMismatch; a.f[DD_AUDIT_FIELD_nBQT] = r->nBQT;
    a.f[DD_AUDIT_FIELD_nmmBQT] = r->nmmBQT; a.f[DD_AUDIT_FIELD_nMMLeft] = r->nMMLeft; a.f[DD_AUDIT_FIELD_nMMRight] = r->nMMRight;
    a.f[DD_AUDIT_FIELD_firstBase] = r->firstBase; a.f[DD_AUDIT_FIELD_lastBase] = r->lastBase; a.f[DD_AUDIT_FIELD_hpos] = r->hpos;
    a.f[DD_AUDIT_FIELD_var_covered] = r->var_covered; a.f[DD_AUDIT_FIELD_var_fcov] = r->var_fcov;
    return a;
}

/* Where one audited pair lies.  j: its index in the shadow (0 ... sizes.n_pairs). */
typedef struct au_pair {
    int32_t w, L, nv;
    int64_t p_pair, s_pair, p_hpos, s_hpos, p_cov, s_cov;     /* first element in the primary / the shadow */
} au_pair;
typedef struct au_geometry {
    int32_t n_windows;
    const int32_t *win_hap_off, *win_read_off, *read_seq_off, *hap_var_off;   /* hap_var_off may be NULL: no variants */
    const int64_t *win_pair_off, *win_hpos_off, *win_varcov_off;              /* the primary's (dd_batch_offsets) */
    const int64_t *pair_off, *hpos_off, *varcov_off;                          /* the shadow's (dd_audit_select) */
} au_geometry;
AU_FN au_pair au_locate(const au_geometry *G, int64_t j)
{
    au_pair a;
    int lo = 0, hi = G->n_windows;                     /* the window with pair_off[w] <= j < pair_off[w + 1]: the last w with pair_off[w] <= j */
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (G->pair_off[mid] <= j) lo = mid; else hi = mid;
    }
    {
        const int w = lo;
        const int64_t local = j - G->pair_off[w];
        const int g0 = G->win_hap_off[w], q0 = G->win_read_off[w], R = G->win_read_off[w + 1] - q0;
        const int h = (int)(local / R), r = (int)(local - (int64_t)h * R);
        const int g = g0 + h, q = q0 + r;
        const int rs0 = G->read_seq_off[q0], SL = G->read_seq_off[q0 + R] - rs0, rb = G->read_seq_off[q];
        const int64_t in_hpos = (int64_t)h * SL + (rb - rs0);
        a.w = w;
        a.L = G->read_seq_off[q + 1] - rb;
        a.nv = G->hap_var_off ? G->hap_var_off[g + 1] - G->hap_var_off[g] : 0;
        a.p_pair = G->win_pair_off[w] + local; a.s_pair = j;
        a.p_hpos = G->win_hpos_off[w] + in_hpos; a.s_hpos = G->hpos_off[w] + in_hpos;
        a.p_cov = a.s_cov = 0;
        if (a.nv > 0) {
            const int64_t in_cov = (int64_t)(G->hap_var_off[g] - G->hap_var_off[g0]) * R + (int64_t)r * a.nv;
            a.p_cov = G->win_varcov_off[w] + in_cov; a.s_cov = G->varcov_off[w] + in_cov;
        }
    }
    return a;
}

#if defined(__cplusplus) && defined(__HIPCC__)
namespace dda {

#define DD_AUDIT_WAVES 4            /* wavefronts per workgroup: one pair in flight per wavefront */
#define DD_AUDIT_MAX_BLOCKS 2048    /* persistent grid: 256 CUs x 8 workgroups; the wavefronts stride over the pairs */

struct AuditArgs {
    au_geometry G;
    au_fields primary, shadow;           /* a field NULL on either side is skipped */
    int32_t has_flank;
    int64_t j_begin, j_end;              /* the audited pairs (shadow indices) this launch covers */
    dd_audit_report *report;
    dd_audit_record *records;
    int64_t max_records;
};
unsigned audit_grid(int64_t n_pairs);
hipError_t launch_audit_compare(const AuditArgs &A, hipStream_t st);

} // namespace dda
#endif
#endif
