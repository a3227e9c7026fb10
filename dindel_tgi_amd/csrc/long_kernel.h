// long_kernel.h — argument block and launchers of the long-window kernel (long_kernel.hip), shared with the host units (capi_internal.h).
#ifndef DD_LONG_KERNEL_H
#define DD_LONG_KERNEL_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dindel_hmm.h"
#include "kernel_common.h"   /* the header words and lists both long paths share: DD_LWS_* */

#define DD_LONG_THREADS 256   /* one workgroup (four wavefronts) per pair */
#define DD_LONG_PAD 32        /* pad states either side of the LDS row: jumps reach D <= 32 states (the wide build clips its loops instead) */

namespace ddl {

/* Workspace of a long launch (dd_workspace_bytes_long):
 *   [0, 256)        header: u64 item counter, i32 long windows, pad, i64 long pairs, u64 stats[2] (pairs computed, most pairs of one workgroup)
 *   [256, ...)      i32 long_win[n_windows]           windows of class DD_WIN_LONG, ascending
 *   [off_lpoff ...) i64 long_pair_off[n_windows + 1]  prefix sums of their pair counts
 *   [off_tiles ...) grid x tile_bytes                 per workgroup: max_read_len rows x 256 K bytes of back-pointers (the wide build: x 2),
 *                                                      2 x 256 K doubles */
#define DD_LONG_HDR_TOTAL 16

struct LongArgs {
    int32_t n_windows, w_begin, w_end;                 /* windows [w_begin, w_end) of the batch are screened for class 2 */
    int32_t read_begin, read_end;                      /* onHap pass: reads [read_begin, read_end) */
    const int32_t *win_hap_off, *win_read_off;
    const uint32_t *win_hap_start;
    const int32_t *hap_seq_off;
    const char *hap_seq;
    const int32_t *hap_var_off, *hap_var, *hap_var_flank;
    const int32_t *read_seq_off;
    const char *read_seq;
    const uint8_t *read_qidx, *read_mqidx;
    const uint32_t *read_start;
    const uint8_t *read_flags;
    const int64_t *win_pair_off, *win_hpos_off, *win_varcov_off;
    const double *tables;
    const uint8_t *sym_lut;
    const uint8_t *win_class;                          /* 2 = long path */
    const int32_t *read_mate_pos, *read_mate_len; const uint8_t *read_lib;
    const int32_t *lib_off; const double *lib_logprob, *lib_log95;
    dd_result out;
    int32_t D, maxLengthDel, padCover, bMid, maxMismatch, n_qual;
    int32_t max_read_len;                              /* rows of a tile; longer reads are not computed (guard) */
    unsigned char *ws;                                 /* workspace (layout above) */
    unsigned long long *stats;                         /* [2]: pairs computed, most pairs one workgroup took */
    uint64_t off_lpoff, off_tiles, tile_bytes, stash_off;   /* a tile: back-pointer rows, then (at stash_off) 2 x 256 K doubles of beta[bMid] */
    uint32_t lds_off_rowI, lds_off_sc, lds_off_hc, lds_off_EN, lds_off_Q, lds_off_lut, lds_off_rdC, lds_off_rdQ, lds_off_ms, lds_off_red;
};

/* LDS bytes of the long kernel for K positions per thread and reads up to max_read_len; fills the offsets of A */
size_t long_lds_layout(int K, int max_read_len, LongArgs &A);
/* what a wide launch does behind its kernel, and all it does for a range without a long window (needs no workspace): the placeholders of
 * the windows of [w_begin, w_end) that are not DD_WIN_LONG, then onHap of every read of [read_begin, read_end) */
hipError_t launch_wide_tail(const LongArgs &A, bool onhap, hipStream_t st);
/* prepass (one workgroup: class-2 windows, pair prefix sums, counter and stats zeroed), the kernel, then onHap of the long windows' reads.
 * wide: the build for maxLengthDel > 31 (two-byte back-pointers), then launch_wide_tail: that launch has no main launch in front of it */
hipError_t launch_long(int K, bool wide, const LongArgs &A, unsigned grid, size_t lds, bool onhap, hipStream_t st);

} // namespace ddl
#endif
