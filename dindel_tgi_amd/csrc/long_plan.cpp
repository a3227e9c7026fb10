// long_plan.cpp — the plans of the two long-window paths of the C ABI and their workspace sizes.  Host arithmetic like plan.cpp, apart from it
// because it needs the LDS and tile layouts that the long kernel units define (ddl::long_lds_layout, ddf::fl_lds_layout, ddf::fl_tile_layout).
#include "capi_internal.h"

namespace ddh {
// header + window list + prefix list of a long workspace (kernel_common.h): where the prefix list and the tiles start
static uint64_t al256(uint64_t v) { return (v + 255u) & ~(uint64_t)255u; }
static void long_list_layout(int n_windows, uint64_t &off_prefix, uint64_t &off_tiles)
{
    off_prefix = al256(DD_LWS_HEADER + 4 * (uint64_t)std::max(n_windows, 1));
    off_tiles = al256(off_prefix + 8 * (uint64_t)(std::max(n_windows, 0) + 1));
}

// ---------------- long windows of the main model (long_kernel.hip) ----------------
// Plan of a long launch: K states per thread (numS <= 256 K, K = 1, 2, 4, 8, 16), LDS, and the persistent grid: the chip's resident
// workgroups (LDS- and register-limited: 2 per CU, 1 at K = 16), shrunk so that header + lists + one back-pointer tile per workgroup stay
// within DD_LONG_WS_BUDGET.  wide: the build for maxLengthDel > 31, whose back-pointer fields take two bytes (32 MiB + stash at the maximum shape).
int long_plan(int n_windows, int max_hap_len, int max_read_len, int n_qual, LongPlan &lp, ddl::LongArgs &A, bool wide)
{
    if (max_hap_len < 1 || max_hap_len > DD_LONG_MAX_HAP_LEN) return fail(DD_ERR_UNSUPPORTED, "long path: haplotype length outside [1,4094]");
    if (max_read_len < 1 || max_read_len > DD_LONG_MAX_READ_LEN) return fail(DD_ERR_UNSUPPORTED, "long path: read length outside [1,4096]");
    const int numS = max_hap_len + 2;
    lp.K = 1;
    while (DD_LONG_THREADS * lp.K < numS) lp.K *= 2;
    A.n_qual = n_qual;
    lp.lds = ddl::long_lds_layout(lp.K, max_read_len, A);
    if (lp.lds + 64 > kCuLdsBytes) return fail(DD_ERR_UNSUPPORTED, "long path: LDS layout too large");
    const unsigned per_cu = std::max(1u, std::min(lp.K >= 16 ? 1u : 2u, (unsigned)((kCuLdsBytes) / (lp.lds + 64))));
    long_list_layout(n_windows, lp.off_lpoff, lp.off_tiles);
    lp.stash_off = al256((uint64_t)max_read_len * DD_LONG_THREADS * lp.K * (wide ? 2 : 1));
    lp.tile_bytes = lp.stash_off + 16 * (uint64_t)DD_LONG_THREADS * lp.K;
    uint64_t grid = (uint64_t)kCUs * per_cu;
    const uint64_t fit = DD_LONG_WS_BUDGET > lp.off_tiles ? (DD_LONG_WS_BUDGET - lp.off_tiles) / lp.tile_bytes : 0;
    if (grid > fit) grid = fit;
    if (grid < 1) grid = 1;
    lp.grid = (unsigned)grid;
    lp.ws_bytes = lp.off_tiles + grid * lp.tile_bytes;
    return DD_SUCCESS;
}

// ---------------- long windows of the --faster model (faster_long_kernel.hip) ----------------
// Plan of a launch: LDS for the shape, and the persistent grid: the chip's resident workgroups (LDS-limited, at most 2 per CU: the kernel is
// built for 2 waves per SIMD), no more than the batch can have 16-pair items, shrunk so that header + lists + 16 tiles per workgroup stay
// within DD_FASTER_LONG_WS_BUDGET.
int fl_plan(const dd_device_batch *b, FLPlan &fp, ddf::FLArgs &A)
{
    const int mh = b->long_max_hap_len, mr = b->long_max_read_len;
    if (mh < 1 || mh > DD_LONG_MAX_HAP_LEN) return fail(DD_ERR_UNSUPPORTED, "--faster long path: haplotype length outside [1,4094]");
    if (mr < 1 || mr > DD_LONG_MAX_READ_LEN) return fail(DD_ERR_UNSUPPORTED, "--faster long path: read length outside [1,4096]");
    A.n_qual = b->n_qual;
    A.max_hap_len = mh; A.max_read_len = mr;
    fp.lds = ddf::fl_lds_layout(mh, mr, A);
    if (fp.lds + 64 > kCuLdsBytes) return fail(DD_ERR_UNSUPPORTED, "--faster long path: LDS layout too large");
    const unsigned per_cu = std::max(1u, std::min(2u, (unsigned)((kCuLdsBytes) / (fp.lds + 64))));
    long_list_layout(b->n_windows, fp.off_ioff, fp.off_tiles);
    const uint64_t wg_bytes = DD_FL_PAIRS * ddf::fl_tile_layout(mh, mr, A);
    uint64_t grid = (uint64_t)kCUs * per_cu;
    const uint64_t items = (uint64_t)std::max(b->n_haps, 0) * (((uint64_t)std::max(b->n_reads, 0) + DD_FL_PAIRS - 1) / DD_FL_PAIRS);
    if (grid > items) grid = items;
    const uint64_t fit = DD_FASTER_LONG_WS_BUDGET > fp.off_tiles ? (DD_FASTER_LONG_WS_BUDGET - fp.off_tiles) / wg_bytes : 0;
    if (grid > fit) grid = fit;
    if (grid < 1) grid = 1;
    fp.grid = (unsigned)grid;
    fp.ws_bytes = fp.off_tiles + grid * wg_bytes;
    A.off_ioff = fp.off_ioff; A.off_tiles = fp.off_tiles; A.grid = (int32_t)grid;
    return DD_SUCCESS;
}
} // namespace ddh
using namespace ddh;
extern "C" {
size_t dd_workspace_bytes_long(const dd_params *p, const dd_device_batch *b)
{
    (void)p;
    if (!b || b->long_max_hap_len <= 0 || b->long_max_read_len <= 0) return 0;
    ddl::LongArgs A;
    memset(&A, 0, sizeof(A));
    LongPlan lp;
    if (long_plan(b->n_windows, b->long_max_hap_len, b->long_max_read_len, b->n_qual, lp, A)) return 0;
    return (size_t)lp.ws_bytes;
}

size_t dd_workspace_bytes_wide(const dd_params *p, const dd_device_batch *b)
{
    if (!p || check_params(p, DD_OPT_WIDE_DELETIONS) != DD_SUCCESS) return 0;
    if (p->maxLengthDel <= DD_MAX_LENGTH_DEL) return dd_workspace_bytes_long(p, b);
    if (!b || b->long_max_hap_len <= 0 || b->long_max_read_len <= 0) return 0;
    ddl::LongArgs A;
    memset(&A, 0, sizeof(A));
    LongPlan lp;
    if (long_plan(b->n_windows, b->long_max_hap_len, b->long_max_read_len, b->n_qual, lp, A, true)) return 0;
    return (size_t)lp.ws_bytes;
}

size_t dd_workspace_bytes_faster_long(const dd_params *p, const dd_device_batch *b)
{
    (void)p;
    if (!b || b->long_max_hap_len <= 0 || b->long_max_read_len <= 0) return 0;
    ddf::FLArgs A;
    memset(&A, 0, sizeof(A));
    FLPlan fp;
    if (fl_plan(b, fp, A)) return 0;
    return (size_t)fp.ws_bytes;
}
} // extern "C"
