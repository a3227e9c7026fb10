/* faster_shadow.h — the "--faster" model (ObservationModelS) written once more, for the audit of --faster launches (include/dindel_hmm.h,
 * "audit of the --faster model").  Plain C++ for host and device: the shadow kernel (faster_shadow_kernel.hip) and the CPU
 * evaluation (faster_shadow_host.cpp, dd_audit_shadow_faster_host) call the same functions; the rule (au_compared_faster) is C99 as well.
 *
 * Written from the reference (Faster.cpp:42-681, Haplotype.hpp:315-384, DInDel.cpp:1790-1833 and 1951-2054), not from the project's two
 * --faster kernels, whose text (their shared model header and its two fragments) this file neither includes nor repeats.  What it does share with
 * them, and what an audit therefore cannot see: the table block of dd_build_tables and its layout (hmm_kernel.h: TC_FAST, T_QUAL's eq /
 * uq, T_MAPQF), the index arrays and the batch, and the rule below.
 *
 * The model is in DESTINATION form: the reference pushes candidates source state by source state (Faster.cpp:373-416, 422-466); here one
 * call computes ONE destination state of one read base and offers it the candidates in the order the reference's source-major loops
 * offer them to that state, each folded with `nv > cur + 1e-7`.  Arithmetic is add, compare, select and (|d| - 1) * (-0.25), in the
 * reference's term order; every logarithm comes from the tables.
 *
 * States of a pair: S <= 16 diagonals rel[0 .. S) (relative positions hx - x, ascending; the sentinel -L among them), state t < S is
 * "on diagonal t", state S + t "inserted at diagonal t".
 */
#ifndef DD_FASTER_SHADOW_H
#define DD_FASTER_SHADOW_H
#include <stdint.h>
#include "../../include/dindel_hmm.h"
#include "audit_kernel.h"    /* au_load, au_field_size, au_fields, au_geometry, au_locate: shared with the main model's audit */

#ifdef __HIPCC__
#define FS_FN static __host__ __device__ __forceinline__
#else
#define FS_FN static inline
#endif

#define FS_KMER 4
#define FS_MAX_DIAGONALS 15                 /* chosen by vote; with the sentinel S <= 16 */
#define FS_MAX_STATES 32                    /* 2 S */
#define FS_EPS 1e-7
#define FS_UNSET (-1000.0)                  /* alpha before any candidate (Faster.cpp:270) */
#define FS_COV_WORDS 128                    /* one bit per haplotype base, DD_LONG_MAX_HAP_LEN bases at most */

/* ---- the rule: what an audit of this model compares for a pair whose two statuses are both `status` ----------------------------------
 * Read off the stores of the two --faster kernels: a pair they do not compute (DD_PAIR_NAN: read shorter than a k-mer; DD_PAIR_HAPSIZE)
 * gets its status, ll = 0, the eleven fields the model leaves at defaults and zeroed coverage flags, and NOTHING in firstBase, lastBase
 * and hpos, which are therefore not read for it. */
FS_FN uint32_t au_compared_faster(int status, int has_flank)
{
    const uint32_t st = 1u << DD_AUDIT_FIELD_status;
    const uint32_t cov = (1u << DD_AUDIT_FIELD_var_covered) | (has_flank ? 1u << DD_AUDIT_FIELD_var_fcov : 0u);
    if (status == DD_PAIR_OK) return ((1u << DD_AUDIT_N_PAIR_FIELDS) - 1u) | (1u << DD_AUDIT_FIELD_hpos) | cov;
    if (status == DD_PAIR_NAN || status == DD_PAIR_HAPSIZE) {
        uint32_t m = st | (1u << DD_AUDIT_FIELD_ll) | cov;
        int f;
        for (f = DD_AUDIT_FIELD_llOn; f <= DD_AUDIT_FIELD_nMMRight; f++) m |= 1u << f;
        return m;
    }
    return st;
}

#ifdef __cplusplus   /* the model: C++ for host and device (the rule above is C99 as well) */
#include "hmm_kernel.h"      /* the table layout */

/* ---- one pair's inputs ---------------------------------------------------------------------------------------------------------------- */
typedef struct fs_pair {
    const char *hap, *read;
    const uint8_t *qidx;                    /* per read base: index into the quality table */
    const double *T;                        /* dd_build_tables' block */
    const int32_t *rel;                     /* [S] the diagonals, ascending (fs_sort_diagonals) */
    int32_t hlen, L, S, bMid, mqidx;
} fs_pair;

/* status of a pair: Faster.cpp:47 (maxLengthIndel against the haplotype), HapHash::convert's throw for a read shorter than a k-mer */
FS_FN int fs_status(int maxLengthDel, int hlen, int L)
{
    if (maxLengthDel > hlen) return DD_PAIR_HAPSIZE;
    if (L < FS_KMER) return DD_PAIR_NAN;
    return DD_PAIR_OK;
}

/* computeBMid (Faster.cpp:60-88): 0 for a read right of the haplotype, L - 1 for one left of it, else the middle of the overlap */
FS_FN int fs_bmid(uint32_t hapStart, int hlen, uint32_t readStart, int L)
{
    const uint32_t hapEnd = hapStart + (uint32_t)hlen, readEnd = readStart + (uint32_t)L - 1u;
    int m;
    if (readStart > hapEnd) m = 0;
    else if (readEnd < hapStart) m = L - 1;
    else {
        const uint32_t s = hapStart > readStart ? hapStart : readStart, e = hapEnd > readEnd ? readEnd : hapEnd;
        m = ((int)e - (int)s) / 2 + (int)s - (int)readStart;
    }
    if (m < 0) m = 0;
    if (m >= L) m = L - 1;
    return m;
}

/* ---- votes (Faster.cpp:131-189, Haplotype.hpp:364-381) -------------------------------------------------------------------------------- */
FS_FN unsigned fs_base2(char c) { return c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 0u; }     /* A, and everything else, is 0 */
FS_FN unsigned fs_kmer_key(const char *s, int x)
{
    unsigned k = 0;
    int y;
    for (y = 0; y < FS_KMER; y++) k |= fs_base2(s[x + y]) << (2 * y);
    return k;
}
FS_FN int fs_n_read_kmers(int L) { return L - FS_KMER + 1; }                 /* x = 0 ... L - 4 */
FS_FN int fs_n_hap_kmers(int hlen) { return hlen > FS_KMER ? hlen - FS_KMER : 0; }   /* hx = 0 ... hlen - 5: the last one is never hashed */
FS_FN int fs_n_bins(int hlen, int L) { return hlen + L; }                   /* bin of diagonal d = hx - x: d + L */

#if defined(__HIP_DEVICE_COMPILE__)
#define FS_BIN_INC(at) atomicAdd((at), 1)
#define FS_BIT_OR(at, v) atomicOr((at), (v))
#else
#define FS_BIN_INC(at) (++*(at))
#define FS_BIT_OR(at, v) (*(at) |= (v))
#endif
/* the votes of haplotype position hx: one for every read position whose 4-mer is hx's.  rk[x]: the read's keys. */
FS_FN void fs_vote_hap_pos(const char *hap, int hx, const uint8_t *rk, int L, int32_t *hist)
{
    const unsigned hk = fs_kmer_key(hap, hx);
    const int nx = fs_n_read_kmers(L);
    int x;
    for (x = 0; x < nx; x++)
        if (rk[x] == hk) FS_BIN_INC(&hist[hx - x + L]);
}
/* order of the selection: count descending, then relative position ascending; 0 for an empty bin */
FS_FN uint64_t fs_vote_rank(int32_t count, int bin)
{
    return count > 0 ? ((uint64_t)(uint32_t)count << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)bin) : 0u;
}
FS_FN int fs_rank_bin(uint64_t rank) { return (int)(0xFFFFFFFFu - (uint32_t)(rank & 0xFFFFFFFFu)); }
/* rel[0 .. n) chosen diagonals, unsorted: appends the sentinel -L (Faster.cpp:263) and sorts ascending; -> S */
FS_FN int fs_sort_diagonals(int32_t *rel, int n, int L)
{
    int i, j;
    rel[n++] = -L;
    for (i = 1; i < n; i++) {
        const int32_t v = rel[i];
        for (j = i; j > 0 && rel[j - 1] > v; j--) rel[j] = rel[j - 1];
        rel[j] = v;
    }
    return n;
}

/* ---- SStateHMM (Faster.cpp:253-576) --------------------------------------------------------------------------------------------------- */
typedef struct fs_cell { double v; int32_t bp; } fs_cell;

FS_FN double fs_log_match(const fs_pair *P, int r) { return P->T[T_QUAL + 4 * P->qidx[r]]; }
/* obs[r][s] (:286-296): off the haplotype everything matches */
FS_FN double fs_obs(const fs_pair *P, int s, int r)
{
    const int hp = P->rel[s] + r;
    const double *q = P->T + T_QUAL + 4 * P->qidx[r];
    if (hp >= 0 && hp < P->hlen) return P->read[r] == P->hap[hp] ? q[0] : q[1];
    return q[0];
}
/* (|rel[s1] - rel[s2]| - 1) * logpInsgIns (:339-352) */
FS_FN double fs_trI(const fs_pair *P, int s1, int s2)
{
    const int d = P->rel[s1] - P->rel[s2];
    return ((double)(d < 0 ? -d : d) - 1.0) * -0.25;
}
FS_FN void fs_offer(fs_cell *c, double nv, int from)
{
    if (nv > c->v + FS_EPS) { c->v = nv; c->bp = from; }
}

/* Destination state t of read base r < bMid in the sweep from the left; prev: alpha[r - 1][0 .. 2S) (not read for r == 0). */
FS_FN fs_cell fs_left_step(const fs_pair *P, int t, int r, const double *prev)
{
    const int S = P->S;
    const double l1mE = P->T[TC_FAST + 0], lE = P->T[TC_FAST + 1], NI = P->T[TC_FAST + 2], LM = fs_log_match(P, r);
    fs_cell c;
    int cs;
    c.v = FS_UNSET; c.bp = 0;
    if (t < S) {
        for (cs = 0; cs <= t; cs++) {                          /* on-diagonal sources at or below (:380-384) */
            double pv = fs_obs(P, cs, r), nv;
            if (r) pv += prev[cs];
            nv = pv + (cs == t ? l1mE : fs_trI(P, cs, t) + lE);
            fs_offer(&c, nv, cs);
        }
        for (cs = t + 1; cs < S; cs++)                         /* inserted sources above, while their diagonal is still reachable (:404-411) */
            if (P->rel[cs] - r >= P->rel[t]) {
                double nv = LM + fs_trI(P, cs, t) + lE;
                if (r) nv += prev[cs + S];
                fs_offer(&c, nv, cs + S);
            }
    } else {
        double pv = fs_obs(P, t - S, r), nv;
        if (r) pv += prev[t - S];
        fs_offer(&c, pv + NI, t - S);                          /* (:387-391) */
        nv = LM + -0.25;
        if (r) nv += prev[t];
        fs_offer(&c, nv, t);                                   /* (:396-400) */
    }
    return c;
}

/* Destination state t of read base r > bMid in the sweep from the right; next: alpha[r + 1][0 .. 2S) (not read for r == L - 1). */
FS_FN fs_cell fs_right_step(const fs_pair *P, int t, int r, const double *next)
{
    const int S = P->S, inner = r < P->L - 1;
    const double l1mE = P->T[TC_FAST + 0], lE = P->T[TC_FAST + 1], NI = P->T[TC_FAST + 2], LM = fs_log_match(P, r);
    fs_cell c;
    int cs;
    c.v = FS_UNSET; c.bp = 0;
    if (t < S) {
        double pv = fs_obs(P, t, r), nv;
        if (inner) pv += next[t];
        fs_offer(&c, pv + l1mE, t);                            /* own diagonal (:427-431) */
        nv = LM + lE;
        if (inner) nv += next[t + S];
        fs_offer(&c, nv, t + S);                               /* its inserted state (:436-438) */
        for (cs = t + 1; cs < S; cs++) {                       /* on-diagonal sources above (:427-431) */
            pv = fs_obs(P, cs, r);
            if (inner) pv += next[cs];
            fs_offer(&c, pv + (fs_trI(P, cs, t) + lE), cs);
        }
    } else {
        const int ns = t - S;
        double nv;
        for (cs = 0; cs < ns; cs++)                            /* on-diagonal sources below (:453-461) */
            if (P->rel[cs] > P->rel[ns] - r) {
                nv = fs_obs(P, cs, r) + NI + fs_trI(P, cs, ns);
                if (inner) nv += next[cs];
                fs_offer(&c, nv, cs);
            }
        nv = LM + -0.25;
        if (inner) nv += next[t];
        fs_offer(&c, nv, t);                                   /* (:443-447) */
    }
    return c;
}

/* alpha[bMid][xx] (:472-486; hmq: :510-526, the fixed mapping quality 1 - 1e-10).  left, right: this state's value in alpha[bMid - 1] and
 * alpha[bMid + 1] (not read where there is no such base). */
FS_FN double fs_join(const fs_pair *P, int xx, int hmq, double left, double right)
{
    const int ins = xx >= P->S, y = ins ? xx - P->S : xx, hp = P->rel[y] + P->bMid;
    const int on = hp >= 0 && hp < P->hlen;
    const double *T = P->T;
    const double first = hmq ? (on ? T[TC_FAST + 3] : T[TC_FAST + 4]) : (on ? T[T_MAPQF + 2 * P->mqidx] : T[T_MAPQF + 2 * P->mqidx + 1]);
    const double prior = first + (ins ? T[TC_FAST + 1] : T[TC_FAST + 0]);
    double v = (ins ? fs_log_match(P, P->bMid) : fs_obs(P, y, P->bMid)) + prior;
    if (P->bMid < P->L - 1) v += right;
    if (P->bMid > 0) v += left;
    return v;
}

/* The state path (:540-548) from the back-pointers bt[r * FS_MAX_STATES + t], then mapState (:552-571) into ms[0 .. L). */
FS_FN void fs_traceback(const fs_pair *P, const uint8_t *bt, int xmax, uint8_t *path, int16_t *ms)
{
    int r, lhp = 1;
    path[P->bMid] = (uint8_t)xmax;
    for (r = P->bMid; r > 0; r--) path[r - 1] = bt[(r - 1) * FS_MAX_STATES + path[r]];
    for (r = P->bMid; r < P->L - 1; r++) path[r + 1] = bt[(r + 1) * FS_MAX_STATES + path[r]];
    for (r = 0; r < P->L; r++) {
        const int s = path[r];
        int m;
        if (s < P->S) {
            const int hp = P->rel[s] + r;
            if (hp >= 0 && hp < P->hlen) { m = hp + 1; lhp = hp + 1; }
            else m = hp < 0 ? 0 : P->hlen;
        } else m = P->hlen + 2 + lhp;
        ms[r] = (int16_t)m;
    }
}

/* reportVariants (:579-681) for one read base: its hpos entry in the product's encoding; *hb: the haplotype base it is aligned to, or -1 */
FS_FN int fs_hpos_of(int m, int hlen, int *hb)
{
    const int numS = hlen + 2, x = m % numS;
    *hb = -1;
    if (x > 0 && x <= hlen) {
        if (m >= numS) return DD_HPOS_INS_KEY0 - x;            /* inserted: carries its key, the position after the last aligned base */
        *hb = m - 1;
        return m - 1;
    }
    return x == 0 ? DD_HPOS_LO : DD_HPOS_RO;
}
/* AlignedVariant::isCovered (Variant.hpp:125-128) */
FS_FN int fs_var_covered(int firstBase, int lastBase, int padCover, int sR, int eR)
{
    return firstBase + padCover <= sR && lastBase - padCover >= eR;
}
/* filterHaplotypes' test of one read against one indel (DInDel.cpp:1951-2054), in two passes over a bitmap of the haplotype's bases
 * (FS_COV_WORDS words, zeroed by the caller): fs_fcov_base marks the base read position b is aligned to, if it lies in [left, right], and
 * returns 1 for a mismatch there ('N' exempt for a deletion, kind 1); fs_fcov_bit says whether haplotype base x was marked.  Covered:
 * every base of the interval marked and at most maxMismatch mismatches; an interval that reaches outside the haplotype never is. */
FS_FN int fs_fcov_base(const fs_pair *P, const int16_t *ms, int b, int left, int right, int kind, uint32_t *bits)
{
    int hb;
    (void)fs_hpos_of(ms[b], P->hlen, &hb);
    if (hb < 0 || hb < left || hb > right) return 0;
    FS_BIT_OR(&bits[hb >> 5], 1u << (hb & 31));
    if (kind == 1 && P->hap[hb] == 'N') return 0;
    return P->hap[hb] != P->read[b];
}
FS_FN int fs_fcov_bit(const uint32_t *bits, int x) { return (int)(bits[x >> 5] >> (x & 31) & 1u); }

/* ---- where an audited pair's inputs lie ----------------------------------------------------------------------------------------------- */
typedef struct fs_where { au_pair a; int32_t g, q, r; } fs_where;      /* haplotype, read, read's index in its window */
FS_FN fs_where fs_locate(const au_geometry *G, int64_t j)
{
    fs_where x;
    x.a = au_locate(G, j);
    {
        const int w = x.a.w, q0 = G->win_read_off[w], R = G->win_read_off[w + 1] - q0;
        const int64_t local = j - G->pair_off[w];
        const int h = (int)(local / R);
        x.r = (int)(local - (int64_t)h * R);
        x.g = G->win_hap_off[w] + h;
        x.q = q0 + x.r;
    }
    return x;
}

#ifdef __HIPCC__
namespace dfs {

#define DD_FS_WAVES 4               /* wavefronts per workgroup: one pair in flight per wavefront */
#define DD_FS_MAX_BLOCKS 2048       /* persistent grid; the wavefronts stride over the sample's pairs */
#define DD_FS_WS_BUDGET ((size_t)256 << 20)

struct ShadowArgs {
    au_geometry G;                       /* primary offsets unused by the shadow kernel */
    const uint32_t *win_hap_start;
    const int32_t *hap_seq_off; const char *hap_seq;
    const int32_t *hap_var, *hap_var_flank;
    const char *read_seq; const uint8_t *read_qidx, *read_mqidx; const uint32_t *read_start;
    const double *tables;
    dd_result out;                       /* the shadow */
    int32_t maxLengthDel, padCover, maxMismatch;
    int32_t max_hap_len, max_read_len;   /* what the areas are sized for; a longer pair is not computed (guard) */
    int64_t j_begin, j_end;
    unsigned char *ws;                   /* NULL: the areas are in LDS */
    uint32_t area_bytes, off_path, off_ms;   /* one wavefront's area and the parts in it: filled by launch_shadow */
};
/* one wavefront's area: back-pointer tile (over the vote histogram), state path (over the read's keys), mapState */
uint32_t area_bytes(int max_hap_len, int max_read_len);
bool area_in_lds(int max_hap_len, int max_read_len);
unsigned shadow_grid(int64_t n_pairs, int max_hap_len, int max_read_len);
size_t shadow_lds_bytes(int max_hap_len, int max_read_len);
hipError_t launch_shadow(const ShadowArgs &A, hipStream_t st);
/* the comparison under au_compared_faster (dda::AuditArgs as the main model's) */
hipError_t launch_compare_faster(const dda::AuditArgs &A, hipStream_t st);

} // namespace dfs
#endif
#endif /* __cplusplus */
#endif
