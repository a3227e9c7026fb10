// align_host.cpp — host side of the haplotype-to-reference alignment (hapalign_kernel.hip) and of the indel-event and variant extraction
// that run behind an alignment launch (align_events_kernel.hip, hap_variants_kernel.hip): validation of a dd_align_batch, the grid /
// workspace rule, the three device-pointer launches with their launch records, and the one host-pointer entry behind dd_align_haplotypes,
// ..._events and ..._variants: its checks and its list of arrays.  The arena, the records and the copy back are capi_internal.h's.
#include "capi_internal.h"
#include "hapalign_kernel.h"
#include "align_events_kernel.h"
#include "hap_variants_kernel.h"

namespace ddh {
namespace {

struct AlignShape { int64_t ref_bytes, hap_bytes; int max_ref_len, max_hap_len; };

// this thread's last alignment, event and variants launch; the last two keep their words in the header of the alignment workspace they
// ran behind (capi_internal.h: LaunchRecord)
thread_local LaunchRecord g_align_last(DD_ALIGN_LOG_FIELDS), g_events_last(DD_ALIGN_EVENTS_LOG_FIELDS), g_variants_last(DD_ALIGN_EVENTS_LOG_FIELDS);

// offsets start at 0 and never decrease; pair_ref in range.  The maxima leave out what the kernel refuses (too long).
int check_align_batch(const dd_align_batch *b, AlignShape &s)
{
    if (!b) return fail(DD_ERR_INVALID, "null align batch");
    if (b->n_refs < 0 || b->n_pairs < 0) return fail(DD_ERR_INVALID, "negative count in align batch");
    if (!b->ref_off || !b->hap_off) return fail(DD_ERR_INVALID, "null offset array in align batch");
    if (b->n_pairs > 0 && !b->pair_ref) return fail(DD_ERR_INVALID, "null pair_ref in align batch");
    s = AlignShape{0, 0, 0, 0};
    if (b->ref_off[0] != 0) return fail(DD_ERR_INVALID, "ref_off does not start at 0");
    if (b->hap_off[0] != 0) return fail(DD_ERR_INVALID, "hap_off does not start at 0");
    for (int i = 0; i < b->n_refs; i++) {
        const int64_t n = (int64_t)b->ref_off[i + 1] - b->ref_off[i];
        if (n < 0) return fail(DD_ERR_INVALID, "ref_off decreases at reference " + std::to_string(i));
        if (n <= DD_LONG_MAX_HAP_LEN) s.max_ref_len = std::max(s.max_ref_len, (int)n);
    }
    for (int i = 0; i < b->n_pairs; i++) {
        const int64_t n = (int64_t)b->hap_off[i + 1] - b->hap_off[i];
        if (n < 0) return fail(DD_ERR_INVALID, "hap_off decreases at pair " + std::to_string(i));
        if (n <= DD_LONG_MAX_HAP_LEN) s.max_hap_len = std::max(s.max_hap_len, (int)n);
        if (b->pair_ref[i] < 0 || b->pair_ref[i] >= b->n_refs) return fail(DD_ERR_INVALID, "pair_ref out of range at pair " + std::to_string(i));
    }
    s.ref_bytes = b->ref_off[b->n_refs];
    s.hap_bytes = b->hap_off[b->n_pairs];
    if (s.ref_bytes > 0 && !b->ref_seq) return fail(DD_ERR_INVALID, "null ref_seq in align batch");
    if (s.hap_bytes > 0 && !b->hap_seq) return fail(DD_ERR_INVALID, "null hap_seq in align batch");
    s.max_ref_len = std::max(s.max_ref_len, 1);
    s.max_hap_len = std::max(s.max_hap_len, 1);
    return DD_SUCCESS;
}

// workgroups of the full grid: one wavefront per pair up to the persistent grid's size, fewer while the tiles exceed the budget
unsigned align_full_grid(int64_t n_pairs, uint64_t tile_bytes)
{
    const int64_t fit = (int64_t)(DD_ALIGN_WS_BUDGET / (tile_bytes * DD_ALIGN_WAVES));
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(dda::persistent_grid(n_pairs, DD_ALIGN_WAVES, DD_ALIGN_MAX_BLOCKS), fit));
}

} // namespace
} // namespace ddh

using namespace ddh;

extern "C" {

size_t dd_align_workspace_bytes(const dd_align_batch *shape)
{
    AlignShape s;
    if (check_align_batch(shape, s)) return 0;
    const uint64_t tile = dda::align_tile_bytes(s.max_ref_len, s.max_hap_len);
    return DD_ALIGN_WS_HEADER + (size_t)align_full_grid(shape->n_pairs, tile) * DD_ALIGN_WAVES * tile;
}

int dd_align_haplotypes_device(const dd_align_batch *b, const dd_align_result *r, int max_ref_len, int max_hap_len, void *workspace,
                               size_t workspace_bytes, void *stream)
{
    if (!b || !r) return fail(DD_ERR_INVALID, "dd_align_haplotypes_device: null batch or result");
    if (b->n_refs < 0 || b->n_pairs < 0) return fail(DD_ERR_INVALID, "dd_align_haplotypes_device: negative count");
    if (max_ref_len < 1 || max_ref_len > DD_LONG_MAX_HAP_LEN || max_hap_len < 1 || max_hap_len > DD_LONG_MAX_HAP_LEN)
        return fail(DD_ERR_INVALID, "dd_align_haplotypes_device: max_ref_len / max_hap_len outside 1 ... DD_LONG_MAX_HAP_LEN");
    if (b->n_pairs == 0) return DD_SUCCESS;
    if (!b->ref_off || !b->ref_seq || !b->pair_ref || !b->hap_off || !b->hap_seq || !r->score || !r->status || !r->ref_pos)
        return fail(DD_ERR_INVALID, "dd_align_haplotypes_device: null array");
    if (!workspace) return fail(DD_ERR_INVALID, "dd_align_haplotypes_device: null workspace");
    const uint64_t tile = dda::align_tile_bytes(max_ref_len, max_hap_len);
    const uint64_t wg_bytes = tile * DD_ALIGN_WAVES;
    if (workspace_bytes < DD_ALIGN_WS_HEADER + wg_bytes)
        return fail(DD_ERR_INVALID, "dd_align_haplotypes_device: workspace too small for one workgroup (dd_align_workspace_bytes)");
    const unsigned grid = (unsigned)std::min<uint64_t>(align_full_grid(b->n_pairs, tile), (workspace_bytes - DD_ALIGN_WS_HEADER) / wg_bytes);
    dda::AlignArgs A;
    A.n_refs = b->n_refs; A.n_pairs = b->n_pairs;
    A.ref_off = b->ref_off; A.ref_seq = reinterpret_cast<const uint8_t *>(b->ref_seq);
    A.pair_ref = b->pair_ref; A.hap_off = b->hap_off; A.hap_seq = reinterpret_cast<const uint8_t *>(b->hap_seq);
    A.score = r->score; A.status = r->status; A.ref_pos = r->ref_pos;
    A.max_ref_len = max_ref_len; A.max_hap_len = max_hap_len;
    A.K = (max_hap_len + 63) / 64;
    A.ws = static_cast<unsigned char *>(workspace);
    A.tile_bytes = tile;
    g_align_last.note({(int64_t)grid, (int64_t)grid * DD_ALIGN_WAVES, (int64_t)tile, (int64_t)dda::align_lds_bytes(A.K), (int64_t)b->n_pairs,
                       (int64_t)(DD_ALIGN_WS_HEADER + grid * wg_bytes)}, A.ws, DD_ALIGN_HDR_BASE, stream);
    HIP_TRY(dda::launch_hapalign(A, grid, static_cast<hipStream_t>(stream)));
    return DD_SUCCESS;
}

void dd_align_last_launch(int64_t out[DD_ALIGN_LOG_FIELDS]) { g_align_last.copy_out(out); }

int dd_align_events_device(const dd_align_batch *b, const dd_align_result *r, int32_t *n_events, dd_align_events *events, int events_cap,
                           void *stream)
{
    if (!b || !r) return fail(DD_ERR_INVALID, "dd_align_events_device: null batch or result");
    if (b->n_refs < 0 || b->n_pairs < 0) return fail(DD_ERR_INVALID, "dd_align_events_device: negative count");
    if (events_cap < 1 || events_cap > DD_ALIGN_EVENTS_MAX_CAP)
        return fail(DD_ERR_INVALID, "dd_align_events_device: events_cap outside 1 ... DD_ALIGN_EVENTS_MAX_CAP");
    if (b->n_pairs == 0) return DD_SUCCESS;
    if (!b->ref_off || !b->pair_ref || !b->hap_off || !r->status || !r->ref_pos || !n_events || !events)
        return fail(DD_ERR_INVALID, "dd_align_events_device: null array");
    if (reinterpret_cast<uintptr_t>(events) & 7u) return fail(DD_ERR_INVALID, "dd_align_events_device: events must be 8-byte aligned");
    if (!g_align_last.hdr)
        return fail(DD_ERR_INVALID, "dd_align_events_device: no alignment launch of this thread to run behind (its workspace header holds the pair counter)");
    dda::EventsArgs A;
    A.n_refs = b->n_refs; A.n_pairs = b->n_pairs;
    A.ref_off = b->ref_off; A.pair_ref = b->pair_ref; A.hap_off = b->hap_off;
    A.status = r->status; A.ref_pos = r->ref_pos;
    A.n_events = n_events; A.events = events; A.events_cap = events_cap;
    A.hdr = const_cast<unsigned int *>(g_align_last.hdr);
    g_events_last.note({(int64_t)dda::persistent_grid(b->n_pairs, DD_ALIGN_WAVES, DD_ALIGN_MAX_BLOCKS), (int64_t)b->n_pairs}, A.hdr,
                        DD_EVENTS_HDR_BASE, stream);
    HIP_TRY(dda::launch_align_events(A, static_cast<hipStream_t>(stream)));
    return DD_SUCCESS;
}

void dd_align_events_last_launch(int64_t out[DD_ALIGN_EVENTS_LOG_FIELDS]) { g_events_last.copy_out(out); }

int dd_hap_variants_device(const dd_align_batch *b, const dd_align_result *r, dd_hap_variants_summary *summary, dd_hap_variant *variants, int cap,
                           void *stream)
{
    if (!b || !r) return fail(DD_ERR_INVALID, "dd_hap_variants_device: null batch or result");
    if (b->n_refs < 0 || b->n_pairs < 0) return fail(DD_ERR_INVALID, "dd_hap_variants_device: negative count");
    if (cap < 1 || cap > DD_HAP_VARIANTS_MAX_CAP) return fail(DD_ERR_INVALID, "dd_hap_variants_device: cap outside 1 ... DD_HAP_VARIANTS_MAX_CAP");
    if (b->n_pairs == 0) return DD_SUCCESS;
    if (!b->ref_off || !b->ref_seq || !b->pair_ref || !b->hap_off || !b->hap_seq || !r->status || !r->ref_pos || !summary || !variants)
        return fail(DD_ERR_INVALID, "dd_hap_variants_device: null array");
    if (reinterpret_cast<uintptr_t>(variants) & 7u) return fail(DD_ERR_INVALID, "dd_hap_variants_device: variants must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(summary) & 3u) return fail(DD_ERR_INVALID, "dd_hap_variants_device: summary must be 4-byte aligned");
    if (!g_align_last.hdr)
        return fail(DD_ERR_INVALID, "dd_hap_variants_device: no alignment launch of this thread to run behind (its workspace header holds the pair counter)");
    dda::VariantsArgs A;
    A.n_refs = b->n_refs; A.n_pairs = b->n_pairs;
    A.ref_off = b->ref_off; A.ref_seq = reinterpret_cast<const uint8_t *>(b->ref_seq);
    A.pair_ref = b->pair_ref; A.hap_off = b->hap_off; A.hap_seq = reinterpret_cast<const uint8_t *>(b->hap_seq);
    A.status = r->status; A.ref_pos = r->ref_pos;
    A.summary = summary; A.variants = variants; A.cap = cap;
    A.hdr = const_cast<unsigned int *>(g_align_last.hdr);
    g_variants_last.note({(int64_t)dda::persistent_grid(b->n_pairs, DD_ALIGN_WAVES, DD_ALIGN_MAX_BLOCKS), (int64_t)b->n_pairs}, A.hdr,
                          DD_VARIANTS_HDR_BASE, stream);
    HIP_TRY(dda::launch_hap_variants(A, static_cast<hipStream_t>(stream)));
    return DD_SUCCESS;
}

void dd_hap_variants_last_launch(int64_t out[DD_ALIGN_EVENTS_LOG_FIELDS]) { g_variants_last.copy_out(out); }

} // extern "C"

namespace ddh {
namespace {


// One host-pointer call: the alignment alone (dd_align_haplotypes), or with the events or the variants behind it; then the slice comes back
// only where the caller has room for it.
struct AlignRequest {
    const dd_align_batch *b; dd_align_result *r; int device;
    bool events = false;   int32_t *n_events = nullptr; dd_align_events *ev = nullptr; int events_cap = 0;
    bool variants = false; dd_hap_variants_summary *summary = nullptr; dd_hap_variant *va = nullptr; int cap = 0;
};

int align_host_entry(const AlignRequest &q)
{
    const dd_align_batch *b = q.b;
    dd_align_result *r = q.r;
    AlignShape s;
    int rc = check_align_batch(b, s);
    if (rc) return rc;
    if (!r) return fail(DD_ERR_INVALID, "null align result");
    if (b->n_pairs > 0 && (!r->score || !r->status)) return fail(DD_ERR_INVALID, "null score or status in align result");
    if (!q.events && !q.variants && s.hap_bytes > 0 && !r->ref_pos) return fail(DD_ERR_INVALID, "null ref_pos in align result");
    if (q.variants) {
        if (q.cap < 1 || q.cap > DD_HAP_VARIANTS_MAX_CAP) return fail(DD_ERR_INVALID, "cap outside 1 ... DD_HAP_VARIANTS_MAX_CAP");
        if (b->n_pairs > 0 && (!q.summary || !q.va)) return fail(DD_ERR_INVALID, "null summary or variants");
    }
    if (q.events) {
        if (q.events_cap < 1 || q.events_cap > DD_ALIGN_EVENTS_MAX_CAP) return fail(DD_ERR_INVALID, "events_cap outside 1 ... DD_ALIGN_EVENTS_MAX_CAP");
        if (b->n_pairs > 0 && (!q.n_events || !q.ev)) return fail(DD_ERR_INVALID, "null n_events or events");
    }
    if ((rc = use_device(q.device, "no HIP device: the haplotype alignment has no CPU fallback in this library"))) return rc;
    if (b->n_pairs == 0) return DD_SUCCESS;

    // every array of the call once: offsets, sequences, outputs, workspace, and what the events or the variants add
    const size_t ws_bytes = dd_align_workspace_bytes(b);
    const size_t P = (size_t)b->n_pairs, R = (size_t)b->n_refs, ref_bytes = (size_t)s.ref_bytes, hap_bytes = (size_t)s.hap_bytes;
    const size_t ev_bytes = q.events ? P * (size_t)q.events_cap * sizeof(dd_align_events) : 0;
    const size_t va_bytes = q.variants ? P * (size_t)q.cap * sizeof(dd_hap_variant) : 0;
    dd_align_batch db = *b;
    dd_align_result dr;
    unsigned char *ws;
    int32_t *d_nev; dd_align_events *d_ev; dd_hap_variants_summary *d_sum; dd_hap_variant *d_va;
    OneShotArena arena;
    ArenaRecords records(arena, {&g_align_last, &g_variants_last, &g_events_last});
    if ((rc = arena.place({arena_slot(&db.ref_off, (R + 1) * 4, b->ref_off), arena_slot(&db.ref_seq, ref_bytes, b->ref_seq),
                           arena_slot(&db.pair_ref, P * 4, b->pair_ref), arena_slot(&db.hap_off, (P + 1) * 4, b->hap_off),
                           arena_slot(&db.hap_seq, hap_bytes, b->hap_seq), arena_slot(&dr.score, P * 4), arena_slot(&dr.status, P * 4),
                           arena_slot(&dr.ref_pos, hap_bytes * 2), arena_slot(&ws, ws_bytes), arena_slot(&d_nev, q.events ? P * 4 : 0),
                           arena_slot(&d_ev, ev_bytes), arena_slot(&d_sum, q.variants ? P * sizeof(dd_hap_variants_summary) : 0),
                           arena_slot(&d_va, va_bytes)})))
        return rc;
    if ((rc = dd_align_haplotypes_device(&db, &dr, s.max_ref_len, s.max_hap_len, ws, ws_bytes, nullptr))) return rc;
    if (q.events) {
        // records no event reaches stay 0: the caller's array is overwritten as a whole
        HIP_TRY(hipMemsetAsync(d_ev, 0, ev_bytes, nullptr));
        if ((rc = dd_align_events_device(&db, &dr, d_nev, d_ev, q.events_cap, nullptr))) return rc;
    }
    if (q.variants) {
        // records no variant reaches stay 0: the caller's array is overwritten as a whole
        HIP_TRY(hipMemsetAsync(d_va, 0, va_bytes, nullptr));
        if ((rc = dd_hap_variants_device(&db, &dr, d_sum, d_va, q.cap, nullptr))) return rc;
    }
    HIP_TRY(hipStreamSynchronize(nullptr));
    if ((rc = records.read_stats())) return rc;   // the workspace goes with this call
    return download({{r->score, dr.score, P * 4}, {r->status, dr.status, P * 4}, {r->ref_pos, dr.ref_pos, r->ref_pos ? hap_bytes * 2 : 0},
                     {q.n_events, d_nev, q.events ? P * 4 : 0}, {q.ev, d_ev, ev_bytes},
                     {q.summary, d_sum, q.variants ? P * sizeof(dd_hap_variants_summary) : 0}, {q.va, d_va, va_bytes}});
}

} // namespace
} // namespace ddh

extern "C" {

int dd_align_haplotypes(const dd_align_batch *b, dd_align_result *r, int device) { return align_host_entry({b, r, device}); }

int dd_align_haplotypes_events(const dd_align_batch *b, dd_align_result *r, int32_t *n_events, dd_align_events *events, int events_cap, int device)
{
    AlignRequest q = {b, r, device};
    q.events = true; q.n_events = n_events; q.ev = events; q.events_cap = events_cap;
    return align_host_entry(q);
}

int dd_align_haplotypes_variants(const dd_align_batch *b, dd_align_result *r, dd_hap_variants_summary *summary, dd_hap_variant *variants, int cap, int device)
{
    AlignRequest q = {b, r, device};
    q.variants = true; q.summary = summary; q.va = variants; q.cap = cap;
    return align_host_entry(q);
}

} // extern "C"
