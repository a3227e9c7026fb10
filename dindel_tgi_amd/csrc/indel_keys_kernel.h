/* indel_keys_kernel.h — the number of distinct keys a (haplotype, read) pair of the --faster model enters into its record's indel map
 * (liks[h][r].indels.size(), what the reference's window loop reads at DInDel.cpp:3529), from the pair's hpos.
 *
 * The first part of this file is plain C99 and is the definition: the kernel (indel_keys_kernel.hip) and the CPU evaluation
 * (indel_keys_capi.cpp, dd_indel_keys_host) both classify a read base with ik_classify and add its key with ik_add_key, so the two cannot
 * drift apart.  It restates the B.faster branch of WindowLikelihoods::indelCount (host/compute_likelihoods.cpp), which in turn restates
 * rebuildAlignmentFaster and Faster.cpp:553-661:
 *
 *     lhp = 1; b = 0
 *     while b < L:
 *         c = hp[b]
 *         if DD_HPOS_IS_INS(c):   skip the maximal run of such entries; key = c == DD_HPOS_INS ? lhp : DD_HPOS_INS_POS(c)
 *         else:                   if c >= 0: lhp = c + 1, and if b < L-1 and hp[b+1] >= 0 and hp[b+1] - c > 1: key = c + 1
 *                                 b++
 *     result = number of DISTINCT keys
 *
 * The serial walk consumes a run of inserted entries whole and every other entry one by one, so a run starts exactly at an inserted
 * entry whose left neighbour is not one.  With that, what base b contributes depends on (hp[b-1], hp[b]) alone, plus, for a run that
 * starts with the bare code, on the nearest earlier entry with a position.  The step INTO base b is classified (the deletion between
 * b-1 and b is found at b), so a base needs its left neighbour only.  The count does not depend on the order of the keys, nor does
 * "more than 64 of them".  Any int16 content of hp is covered: keys are 1..32768 and all arithmetic is int.
 */
#ifndef DD_INDEL_KEYS_KERNEL_H
#define DD_INDEL_KEYS_KERNEL_H
#include <stdint.h>
#include "../../include/dindel_hmm.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define IK_FN static __host__ __device__ __forceinline__
#else
#define IK_FN static inline
#endif

enum { IK_NONE = 0, IK_RUN_KEYED = 1, IK_RUN_BARE = 2, IK_DEL = 3 };

/* What the step from base b-1 (prev; DD_HPOS_LO for b == 0: neither inserted nor a position) into base b (cur) enters into the map:
 * nothing, an insertion run with the key its first entry carries, an insertion run keyed by lhp (IK_RUN_BARE: *key is not set), or the
 * deletion between the two bases. */
IK_FN int ik_classify(int prev, int cur, int *key)
{
    if (DD_HPOS_IS_INS(cur)) {
        if (DD_HPOS_IS_INS(prev)) return IK_NONE;          /* inside a run */
        if (cur == DD_HPOS_INS) return IK_RUN_BARE;
        *key = DD_HPOS_INS_POS(cur);
        return IK_RUN_KEYED;
    }
    if (prev >= 0 && cur >= 0 && cur - prev > 1) { *key = prev + 1; return IK_DEL; }
    return IK_NONE;
}

/* lhp behind an entry: one past the entry's position if it has one, else unchanged */
IK_FN int ik_lhp_after(int lhp, int c) { return c >= 0 ? c + 1 : lhp; }

/* Add `key` to the list of distinct keys (DD_INDEL_KEYS_CAP entries).  Returns 0, or 1 when the key is new and the list is full. */
IK_FN int ik_add_key(int *keys, int *nk, int key)
{
    int k;
    for (k = 0; k < *nk; k++) if (keys[k] == key) return 0;
    if (*nk == DD_INDEL_KEYS_CAP) return 1;
    keys[(*nk)++] = key;
    return 0;
}

/* One pair on the CPU: hp[0..L) -> the count, or DD_INDEL_KEYS_OVERFLOW. */
IK_FN int ik_count_serial(const int16_t *hp, int L)
{
    int keys[DD_INDEL_KEYS_CAP], nk = 0, lhp = 1, prev = DD_HPOS_LO, b;
    for (b = 0; b < L; b++) {
        const int cur = hp[b];
        int key = 0;
        const int cls = ik_classify(prev, cur, &key);
        if (cls == IK_RUN_BARE) key = lhp;
        if (cls != IK_NONE && ik_add_key(keys, &nk, key)) return DD_INDEL_KEYS_OVERFLOW;
        lhp = ik_lhp_after(lhp, cur);
        prev = cur;
    }
    return nk;
}

#if defined(__cplusplus) && defined(__HIPCC__)
namespace ddi {

#define DD_INDEL_KEYS_WAVES 4          /* wavefronts per workgroup: one pair in flight per wavefront */
#define DD_INDEL_KEYS_MAX_BLOCKS 2048  /* persistent grid: 256 CUs x 8 workgroups; the wavefronts stride over the pairs */

struct IndelKeysArgs {
    int32_t n_windows;
    int64_t pair_begin, pair_end;        /* pairs this launch covers (the window blocks of the host-pointer path); pair_end < 0 = up to win_pair_off[n_windows] */
    int64_t max_pairs;                   /* no fewer than the launch's pairs: sizes the grid */
    const int32_t *win_read_off, *read_seq_off;
    const int64_t *win_pair_off, *win_hpos_off;
    const int16_t *hpos;                 /* as the likelihood kernels write it (dd_result.hpos) */
    const int32_t *pair_status;          /* dd_result.status; NULL = every pair was computed */
    int16_t *out;                        /* one per pair */
};
hipError_t launch_indel_keys(const IndelKeysArgs &A, hipStream_t st);

} // namespace ddi
#endif
#endif
