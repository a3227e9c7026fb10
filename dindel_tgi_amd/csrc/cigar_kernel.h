// cigar_kernel.h — argument block and launcher of the device-side getCIGAR (cigar_kernel.hip), shared with launch.cpp.
#ifndef DD_CIGAR_KERNEL_H
#define DD_CIGAR_KERNEL_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dindel_hmm.h"

namespace ddc {

/* BAM operation codes, as host/cigar.hpp names them */
enum { CIG_MATCH = 0, CIG_INS = 1, CIG_DEL = 2, CIG_SOFT_CLIP = 4 };

#define DD_CIGAR_WAVES 4          /* wavefronts per workgroup: one pair in flight per wavefront */
#define DD_CIGAR_MAX_BLOCKS 2048  /* persistent grid: 256 CUs x 8 workgroups; the wavefronts stride over the pairs */

struct CigarArgs {
    int32_t n_windows;
    int64_t pair_begin, pair_end;        /* pairs this launch covers (the chunks of the host-pointer path); pair_end < 0 = up to win_pair_off[n_windows] */
    int64_t max_pairs;                   /* no fewer than the launch's pairs: sizes the grid */
    const int32_t *win_hap_off, *win_read_off, *hap_seq_off, *read_seq_off;
    const int64_t *win_pair_off, *win_hpos_off;
    const int16_t *hpos;                 /* as the likelihood kernels write it (dd_result.hpos) */
    const int32_t *pair_status;          /* dd_result.status; NULL = every pair was computed */
    const int32_t *hap_ref_pos;          /* per haplotype base, at the haplotype's hap_seq_off */
    const uint8_t *hap_aligned;          /* per haplotype; NULL = all aligned */
    dd_cigar_result out;
    int32_t ops_cap;
};
hipError_t launch_cigars(const CigarArgs &A, hipStream_t st);

} // namespace ddc
#endif
