// faster_long_kernel.h — argument block and launcher of the --faster model's long-window kernel (faster_long_kernel.hip), shared with the host units (capi_internal.h).
#ifndef DD_FASTER_LONG_KERNEL_H
#define DD_FASTER_LONG_KERNEL_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dindel_hmm.h"
#include "kernel_common.h"   /* the header words and lists both long paths share: DD_LWS_* */

#define DD_FL_THREADS 256     /* one workgroup: four wavefronts x four 16-lane groups = 16 pairs at a time, all of ONE haplotype */
#define DD_FL_PAIRS 16
#define DD_FL_MAX_ROUNDS 16   /* an item is one haplotype x up to 16 * rounds consecutive reads of its window */

namespace ddf {

/* Workspace of a launch (dd_workspace_bytes_faster_long):
 *   [0, 256)        header: u64 item counter, i32 long windows, i32 rounds per item, i64 items, i64 pairs,
 *                   u64 stats[4] (pairs computed, most pairs of one workgroup, most items of one workgroup, 0)
 *   [256, ...)      i32 long_win[n_windows]            windows of class DD_WIN_LONG with pairs, ascending
 *   [off_ioff ...)  i64 item_off[n_windows + 1]        prefix sums of their item counts
 *   [off_tiles ...) grid x 16 x tile_bytes             per 16-lane group: back-pointers (16 B per read base), then at tile_off_freq the vote
 *                                                      histogram (two 16-bit bins per word), whose bytes later hold the state path */
#define DD_FL_HDR_ROUNDS 12
#define DD_FL_HDR_ITEMS 16
#define DD_FL_HDR_PAIRS 24

struct FLArgs {
    int32_t n_windows, w_begin, w_end;                 /* windows [w_begin, w_end) of the batch are screened for class DD_WIN_LONG */
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
    const int64_t *win_pair_off, *win_hpos_off, *win_varcov_off;
    const double *tables;
    const uint8_t *win_class;
    dd_result out;
    int32_t maxLengthDel, padCover, maxMismatch, n_qual;
    int32_t max_hap_len, max_read_len;                 /* what the LDS and the tiles are sized for; longer shapes are not computed (guard) */
    int32_t grid;                                      /* the prepass sizes the items so that the grid has several each */
    unsigned char *ws;
    unsigned long long *stats;                         /* [4] */
    uint64_t off_ioff, off_tiles, tile_bytes, tile_off_freq;
    /* LDS: block-shared offsets, then per-pair areas of lds_pair_bytes each at lds_shared_bytes */
    uint32_t lds_off_qt, lds_off_hap, lds_off_bk, lds_off_hpl, lds_off_cnt, lds_off_item, lds_shared_bytes, lds_pair_bytes;
    uint32_t lds_off_rd, lds_off_x, lds_off_srt;
};

/* LDS bytes for the shape; fills the offsets of A (A.n_qual set by the caller) */
size_t fl_lds_layout(int max_hap_len, int max_read_len, FLArgs &A);
/* bytes of one 16-lane group's HBM tile; fills tile_bytes / tile_off_freq */
uint64_t fl_tile_layout(int max_hap_len, int max_read_len, FLArgs &A);
/* prepass (one workgroup: class-2 windows, item prefix sums, counter and stats zeroed), the kernel, then onHap of the long windows' reads */
hipError_t launch_faster_long(const FLArgs &A, unsigned grid, size_t lds, bool onhap, hipStream_t st);

} // namespace ddf
#endif
