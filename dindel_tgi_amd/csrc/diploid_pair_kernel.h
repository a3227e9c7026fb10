// diploid_pair_kernel.h — the certified MAP haplotype pair of a window (maxLikelihoodPair's argmax, host/realigned_bam.cpp, reference
// DInDel.cpp:3767-3831), defined once for the device (diploid_pair_kernel.hip) and the host (diploid_pair_host.cpp).
//
// Per window with H haplotypes and R reads, for every pair h1 <= h2 in row-major order (index p):
//     t_r = pm_add_logs(ll[h1, r], ll[h2, r]) + pm_log(0.5)
//     S = 0; for r = 0 ... R-1 in read order: S = S + t_r; A = A + |t_r|            (dp_acc_add: the one order of the sum)
//     V = S + prior[h1 * H + h2];  eps = 2^-50 ((R + 4) A + 8 R + |prior|)          (dp_value)
// and the two first pairs under the total order "larger V first, smaller p first" (DpTop2; V is never NaN there: a NaN V makes the
// window DD_DIPPAIR_NONFINITE).  That order has no ties, so the two pairs do not depend on the order in which pairs are offered or partial
// results merged: the host offers them serially, the kernel one lane per pair and then across lanes, and both find the same two.
// dp_finish() turns them into the window's outputs.  The arithmetic is pooled_math.h's (bit-equal on host and device); every unit that
// includes this file is compiled with -ffp-contract=off.  DESIGN 23 derives eps.
#ifndef DD_DIPLOID_PAIR_KERNEL_H
#define DD_DIPLOID_PAIR_KERNEL_H
#include <stdint.h>
#include "../../include/dindel_hmm.h"
#include "pooled_math.h"

#define DP_NO_PAIR 0x7fffffff          /* index of "no pair" in a DpTop2: behind every pair */

PM_HD bool dp_finite(double x) { return (pm_bits(x) & 0x7ff0000000000000LL) != 0x7ff0000000000000LL; }

// row-major index p of a pair h1 <= h2 of H haplotypes -> (h1, h2); p < H (H + 1) / 2
PM_HD void dp_pair_of_index(int H, int p, int &h1, int &h2)
{
    int row = 0;
    while (p >= H - row) { p -= H - row; row++; }
    h1 = row; h2 = row + p;
}

struct DpAcc { double S, A; };
PM_HD void dp_acc_clear(DpAcc &a) { a.S = 0.0; a.A = 0.0; }
// the next read of a pair's sum, in read order
PM_HD void dp_acc_add(DpAcc &a, double l1, double l2, double log_half)
{
    const double t = pm_add_logs(l1, l2) + log_half;
    a.S = a.S + t;
    a.A = a.A + pm_abs(t);
}
PM_HD void dp_value(const DpAcc &a, int R, double prior, double &V, double &eps)
{
    V = a.S + prior;
    eps = 0x1p-50 * (((double)(R + 4) * a.A + 8.0 * (double)R) + pm_abs(prior));
}

// the first two pairs in the order (V descending, index ascending)
struct DpTop2 { double v1, e1, v2, e2; int32_t p1, p2; };
PM_HD void dp_top2_clear(DpTop2 &t) { t.v1 = t.v2 = -pm_inf(); t.e1 = t.e2 = 0.0; t.p1 = t.p2 = DP_NO_PAIR; }
PM_HD bool dp_before(double va, int32_t pa, double vb, int32_t pb) { return va > vb || (va == vb && pa < pb); }
PM_HD void dp_top2_offer(DpTop2 &t, double v, double e, int32_t p)
{
    if (dp_before(v, p, t.v1, t.p1)) { t.v2 = t.v1; t.e2 = t.e1; t.p2 = t.p1; t.v1 = v; t.e1 = e; t.p1 = p; }
    else if (dp_before(v, p, t.v2, t.p2)) { t.v2 = v; t.e2 = e; t.p2 = p; }
}
PM_HD void dp_top2_merge(DpTop2 &t, const DpTop2 &o)
{
    dp_top2_offer(t, o.v1, o.e1, o.p1);
    dp_top2_offer(t, o.v2, o.e2, o.p2);
}

// One window's outputs.  early: a state found before any sum was taken (DD_DIPPAIR_NO_HAPS, _TOO_MANY_HAPS, _NOT_COMPUTED, _NONFINITE), or
// DD_DIPPAIR_CERTIFIED when the sums ran; any_nan: some pair's V was NaN.  Every state but DD_DIPPAIR_CERTIFIED and DD_DIPPAIR_TIE writes
// best = gap = margin = 0; every state but DD_DIPPAIR_CERTIFIED writes the pair (-1, -1).
PM_HD void dp_finish(int H, int early, bool any_nan, const DpTop2 &t, int32_t *pair, int32_t *state, double *best, double *gap, double *margin)
{
    int st = early;
    double b = 0.0, g = 0.0, m = 0.0;
    int h1 = -1, h2 = -1;
    if (st == DD_DIPPAIR_CERTIFIED) {
        if (any_nan || t.p1 == DP_NO_PAIR || !dp_finite(t.v1)) {
            st = DD_DIPPAIR_NONFINITE;
        } else {
            b = t.v1;
            g = t.p2 == DP_NO_PAIR ? pm_inf() : t.v1 - t.v2;
            m = t.e2 > t.e1 ? t.e2 : t.e1;
            if (g > m) dp_pair_of_index(H, t.p1, h1, h2); else st = DD_DIPPAIR_TIE;
        }
    }
    pair[0] = h1; pair[1] = h2; *state = st; *best = b; *gap = g; *margin = m;
}

#if defined(__HIPCC__)
namespace ddq {
struct DiploidPairArgs {
    int32_t n_windows;
    const int32_t *win_hap_off, *win_read_off;
    const int64_t *win_pair_off, *win_hh_off;
    const double *ll, *prior;
    const int32_t *status;               // NULL = every pair was computed
    dd_diploid_pair_result out;
};
constexpr int kReadChunk = 16;           // reads of every haplotype staged in LDS at a time
constexpr int kMaxBlocks = 2048;         // persistent grid: one wavefront per workgroup, the workgroups stride over the windows
hipError_t launch_diploid_pairs(const DiploidPairArgs &A, hipStream_t st);
} // namespace ddq
#endif

namespace ddh {
// diploid_pair_host.cpp: offsets, arrays and outputs of a batch checked (host pointers)
int check_diploid_pairs(const dd_batch *b, const double *ll, const double *prior, const dd_diploid_pair_result *out);
// diploid_pair_capi.cpp: the pair launch over the windows [w0, w1) of the batch (the window blocks of the host-pointer path); w1 < 0 = all of
// them.  Device pointers, each the whole batch's array.
int launch_diploid_pairs_range(const dd_device_batch *b, const int64_t *win_hh_off_dev, const double *ll_dev, const int32_t *status_dev,
                               const double *prior_dev, const dd_diploid_pair_result *out_dev, void *stream, int w0, int w1);
}
#endif
