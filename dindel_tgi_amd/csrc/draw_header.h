// draw_header.h — what the kernels whose wavefronts draw their items from a counter share (hapalign, align_events, hap_variants, hapdist):
// the three u32 words each launch keeps in a workspace header, where those words live, the grid rule and the launch sequence.  The draw
// loops themselves stay as text in their kernels.
#ifndef DD_DRAW_HEADER_H
#define DD_DRAW_HEADER_H
#include <hip/hip_runtime.h>
#include <stdint.h>

/* the words of one launch, from its base word on */
#define DD_DRAW_COUNTER 0             /* u32 item counter: every wavefront draws its next item from it */
#define DD_DRAW_MAX_DRAWS 1           /* most items one wavefront drew */
#define DD_DRAW_TRIPS 2               /* wavefronts that left through the draw guard (more draws than the launch has items): 0 */
#define DD_DRAW_WORDS 3

/* The alignment workspace starts with a header of DD_ALIGN_WS_HEADER bytes (the trace tiles follow).  The event launch and the variants
 * launch run behind an alignment launch and keep their words in its header, each at a base word of its own; the block table has a
 * workspace of its own (DD_HAPDIST_WS_BYTES, hapdist_kernel.h). */
#define DD_ALIGN_WS_HEADER 256
#define DD_ALIGN_HDR_BASE 0
#define DD_EVENTS_HDR_BASE 4
#define DD_VARIANTS_HDR_BASE 8
#define DD_HAPDIST_HDR_BASE 0
static_assert(DD_ALIGN_HDR_BASE + DD_DRAW_WORDS <= DD_EVENTS_HDR_BASE && DD_EVENTS_HDR_BASE + DD_DRAW_WORDS <= DD_VARIANTS_HDR_BASE &&
                  4 * (DD_VARIANTS_HDR_BASE + DD_DRAW_WORDS) <= DD_ALIGN_WS_HEADER,
              "the three launches behind an alignment keep their words apart, inside its workspace header");

#define DD_ALIGN_HDR_COUNTER (DD_ALIGN_HDR_BASE + DD_DRAW_COUNTER)
#define DD_ALIGN_HDR_MAX_DRAWS (DD_ALIGN_HDR_BASE + DD_DRAW_MAX_DRAWS)
#define DD_ALIGN_HDR_TRIPS (DD_ALIGN_HDR_BASE + DD_DRAW_TRIPS)
#define DD_EVENTS_HDR_COUNTER (DD_EVENTS_HDR_BASE + DD_DRAW_COUNTER)
#define DD_EVENTS_HDR_MAX_DRAWS (DD_EVENTS_HDR_BASE + DD_DRAW_MAX_DRAWS)
#define DD_EVENTS_HDR_TRIPS (DD_EVENTS_HDR_BASE + DD_DRAW_TRIPS)
#define DD_VARIANTS_HDR_COUNTER (DD_VARIANTS_HDR_BASE + DD_DRAW_COUNTER)
#define DD_VARIANTS_HDR_MAX_DRAWS (DD_VARIANTS_HDR_BASE + DD_DRAW_MAX_DRAWS)
#define DD_VARIANTS_HDR_TRIPS (DD_VARIANTS_HDR_BASE + DD_DRAW_TRIPS)
#define DD_HAPDIST_HDR_COUNTER (DD_HAPDIST_HDR_BASE + DD_DRAW_COUNTER)
#define DD_HAPDIST_HDR_MAX_DRAWS (DD_HAPDIST_HDR_BASE + DD_DRAW_MAX_DRAWS)
#define DD_HAPDIST_HDR_TRIPS (DD_HAPDIST_HDR_BASE + DD_DRAW_TRIPS)

namespace dda {

/* workgroups of a persistent grid: one wavefront per item, `waves` per workgroup, at least one workgroup and at most max_blocks */
inline unsigned persistent_grid(int64_t n, int waves, int max_blocks)
{
    const int64_t blocks = (n + waves - 1) / waves;
    return (unsigned)(blocks < 1 ? 1 : blocks > max_blocks ? max_blocks : blocks);
}

#ifdef __HIPCC__
/* zero `zero_bytes` of the header at `zero` on the stream, launch behind that, and say what the launch left */
template <class Args>
inline hipError_t zero_and_launch(void (*kernel)(Args), unsigned grid, unsigned threads, size_t lds, void *zero, size_t zero_bytes, hipStream_t st,
                                  const Args &A)
{
    const hipError_t e = hipMemsetAsync(zero, 0, zero_bytes, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, st, A);
    return hipGetLastError();
}
#endif

} // namespace dda
#endif
