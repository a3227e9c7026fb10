// align_events_kernel.h — argument block and launcher of the indel-event extraction (align_events_kernel.hip), shared with align_host.cpp.
#ifndef DD_ALIGN_EVENTS_KERNEL_H
#define DD_ALIGN_EVENTS_KERNEL_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hapalign_kernel.h"

namespace dda {

/* The event launch runs behind an alignment launch and keeps its three words DD_EVENTS_HDR_* in that launch's workspace header
 * (draw_header.h): zeroed on the stream in front of the event launch. */

struct EventsArgs {
    int32_t n_refs, n_pairs;
    const int32_t *ref_off;              /* [n_refs + 1]: the reference length decides INS against RO */
    const int32_t *pair_ref, *hap_off;   /* [n_pairs], [n_pairs + 1] */
    const int32_t *status;               /* [n_pairs] as the alignment left it */
    const int16_t *ref_pos;              /* laid out like hap_seq */
    int32_t *n_events;                   /* [n_pairs] */
    dd_align_events *events;             /* [n_pairs * events_cap] */
    int32_t events_cap;
    unsigned int *hdr;                   /* the alignment workspace's header, as u32 words */
};

hipError_t launch_align_events(const EventsArgs &A, hipStream_t st);

} // namespace dda
#endif
