// hapalign_kernel.h — argument block and launcher of the haplotype-to-reference alignment (hapalign_kernel.hip), shared with align_host.cpp.
#ifndef DD_HAPALIGN_KERNEL_H
#define DD_HAPALIGN_KERNEL_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dindel_hmm.h"
#include "draw_header.h"

namespace dda {

#define DD_ALIGN_WAVES 4              /* wavefronts per workgroup: one pair in flight per wavefront */
#define DD_ALIGN_MAX_BLOCKS 2048      /* persistent grid: 256 CUs x 8 workgroups; the wavefronts draw pairs from a counter */
#define DD_ALIGN_WS_BUDGET (512ull << 20)   /* the grid shrinks so the tiles stay within this (like DD_LONG_WS_BUDGET), never below one workgroup */

/* Workspace of a launch (dd_align_workspace_bytes):
 *   [0, 256)     header (DD_ALIGN_WS_HEADER, draw_header.h): the alignment's three words DD_ALIGN_HDR_* and those of the launches that
 *                run behind it; zeroed on the stream in front of the launch
 *   [256, ...)   grid x DD_ALIGN_WAVES tiles of tile_bytes: one byte per DP cell of the wavefront's current pair, stored by anti-diagonal
 *                step t = (column - 1) + (lane of the row): byte t * len2 + (row - 1); t < len1 + 63, so a tile of
 *                (max_ref_len + 64) * max_hap_len bytes holds every pair the launch admits */
struct AlignArgs {
    int32_t n_refs, n_pairs;
    const int32_t *ref_off;              /* [n_refs + 1] */
    const uint8_t *ref_seq;
    const int32_t *pair_ref, *hap_off;   /* [n_pairs], [n_pairs + 1] */
    const uint8_t *hap_seq;
    int32_t *score, *status;             /* [n_pairs] */
    int16_t *ref_pos;                    /* laid out like hap_seq */
    int32_t max_ref_len, max_hap_len;    /* longer pairs are DD_ALIGN_TOO_LONG: they size the tile and the LDS rows */
    int32_t K;                           /* ceil(max_hap_len / 64): LDS rows per lane */
    unsigned char *ws;
    uint64_t tile_bytes;
};

inline uint64_t align_tile_bytes(int max_ref_len, int max_hap_len)
{
    const uint64_t b = (uint64_t)(max_ref_len + 64) * (uint64_t)max_hap_len;
    return (b + 255u) & ~uint64_t(255u);
}
/* LDS bytes of a workgroup: per wavefront and haplotype row one int32 each of the mat and horizontal columns and the row's base code */
inline size_t align_lds_bytes(int K) { return (size_t)DD_ALIGN_WAVES * 64u * (size_t)K * 9u; }
hipError_t launch_hapalign(const AlignArgs &A, unsigned grid, hipStream_t st);

} // namespace dda
#endif
