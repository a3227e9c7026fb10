// align_host.cpp — host side of the haplotype-to-reference alignment (hapalign_kernel.hip): validation of a dd_align_batch, the grid /
// workspace rule, the device-pointer launch and the host-pointer entry (its own allocations: one call per batch of windows); and the same
// three for the indel-event extraction and for the variant extraction that run behind an alignment launch (align_events_kernel.hip,
// hap_variants_kernel.hip).
#include "capi_internal.h"
#include "hapalign_kernel.h"
#include "align_events_kernel.h"
#include "hap_variants_kernel.h"

namespace ddh {
namespace {

struct AlignShape { int64_t ref_bytes, hap_bytes; int max_ref_len, max_hap_len; };

// this thread's last launch: the host-side fields, and where its two device words are (read on demand, or cached by the host entry,
// whose workspace does not outlive the call)
struct AlignLast { int64_t v[DD_ALIGN_LOG_FIELDS]; const unsigned char *ws; hipStream_t stream; bool have_stats; };
thread_local AlignLast g_align_last = {{0, 0, 0, 0, 0, 0, 0, 0}, nullptr, nullptr, true};

// this thread's last event launch; its device words are in the header of the alignment workspace it ran behind
struct EventsLast { int64_t v[DD_ALIGN_EVENTS_LOG_FIELDS]; const unsigned char *ws; hipStream_t stream; bool have_stats; };
thread_local EventsLast g_events_last = {{0, 0, 0, 0}, nullptr, nullptr, true};

int read_events_stats()
{
    EventsLast &L = g_events_last;
    if (L.have_stats || !L.ws) return DD_SUCCESS;
    uint32_t hdr[3];
    HIP_TRY(hipStreamSynchronize(L.stream));
    HIP_TRY(hipMemcpy(hdr, L.ws + 4 * DD_EVENTS_HDR_COUNTER, sizeof(hdr), hipMemcpyDeviceToHost));
    L.v[2] = hdr[DD_EVENTS_HDR_MAX_DRAWS - DD_EVENTS_HDR_COUNTER]; L.v[3] = hdr[DD_EVENTS_HDR_TRIPS - DD_EVENTS_HDR_COUNTER];
    L.have_stats = true;
    return DD_SUCCESS;
}

// this thread's last variants launch, likewise
thread_local EventsLast g_variants_last = {{0, 0, 0, 0}, nullptr, nullptr, true};

int read_variants_stats()
{
    EventsLast &L = g_variants_last;
    if (L.have_stats || !L.ws) return DD_SUCCESS;
    uint32_t hdr[3];
    HIP_TRY(hipStreamSynchronize(L.stream));
    HIP_TRY(hipMemcpy(hdr, L.ws + 4 * DD_VARIANTS_HDR_COUNTER, sizeof(hdr), hipMemcpyDeviceToHost));
    L.v[2] = hdr[DD_VARIANTS_HDR_MAX_DRAWS - DD_VARIANTS_HDR_COUNTER]; L.v[3] = hdr[DD_VARIANTS_HDR_TRIPS - DD_VARIANTS_HDR_COUNTER];
    L.have_stats = true;
    return DD_SUCCESS;
}

int read_align_stats()
{
    AlignLast &L = g_align_last;
    if (L.have_stats || !L.ws) return DD_SUCCESS;
    uint32_t hdr[4];
    HIP_TRY(hipStreamSynchronize(L.stream));
    HIP_TRY(hipMemcpy(hdr, L.ws, sizeof(hdr), hipMemcpyDeviceToHost));
    L.v[6] = hdr[DD_ALIGN_HDR_MAX_DRAWS]; L.v[7] = hdr[DD_ALIGN_HDR_TRIPS];
    L.have_stats = true;
    return DD_SUCCESS;
}

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
    int64_t blocks = std::max<int64_t>(1, (n_pairs + DD_ALIGN_WAVES - 1) / DD_ALIGN_WAVES);
    blocks = std::min<int64_t>(blocks, DD_ALIGN_MAX_BLOCKS);
    const int64_t fit = (int64_t)(DD_ALIGN_WS_BUDGET / (tile_bytes * DD_ALIGN_WAVES));
    return (unsigned)std::max<int64_t>(1, std::min(blocks, fit));
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
    const int64_t rec[DD_ALIGN_LOG_FIELDS] = {(int64_t)grid, (int64_t)grid * DD_ALIGN_WAVES, (int64_t)tile, (int64_t)dda::align_lds_bytes(A.K),
                                              (int64_t)b->n_pairs, (int64_t)(DD_ALIGN_WS_HEADER + grid * wg_bytes), -1, -1};
    memcpy(g_align_last.v, rec, sizeof(rec));
    g_align_last.ws = A.ws; g_align_last.stream = static_cast<hipStream_t>(stream); g_align_last.have_stats = false;
    HIP_TRY(dda::launch_hapalign(A, grid, static_cast<hipStream_t>(stream)));
    return DD_SUCCESS;
}

void dd_align_last_launch(int64_t out[DD_ALIGN_LOG_FIELDS])
{
    (void)read_align_stats();                  // a failure leaves -1 in the two device fields
    if (out) memcpy(out, g_align_last.v, sizeof(g_align_last.v));
}

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
    if (!g_align_last.ws)
        return fail(DD_ERR_INVALID, "dd_align_events_device: no alignment launch of this thread to run behind (its workspace header holds the pair counter)");
    dda::EventsArgs A;
    A.n_refs = b->n_refs; A.n_pairs = b->n_pairs;
    A.ref_off = b->ref_off; A.pair_ref = b->pair_ref; A.hap_off = b->hap_off;
    A.status = r->status; A.ref_pos = r->ref_pos;
    A.n_events = n_events; A.events = events; A.events_cap = events_cap;
    A.hdr = reinterpret_cast<unsigned int *>(const_cast<unsigned char *>(g_align_last.ws));
    const int64_t rec[DD_ALIGN_EVENTS_LOG_FIELDS] = {(int64_t)dda::events_grid(b->n_pairs), (int64_t)b->n_pairs, -1, -1};
    memcpy(g_events_last.v, rec, sizeof(rec));
    g_events_last.ws = g_align_last.ws; g_events_last.stream = static_cast<hipStream_t>(stream); g_events_last.have_stats = false;
    HIP_TRY(dda::launch_align_events(A, static_cast<hipStream_t>(stream)));
    return DD_SUCCESS;
}

void dd_align_events_last_launch(int64_t out[DD_ALIGN_EVENTS_LOG_FIELDS])
{
    (void)read_events_stats();                 // a failure leaves -1 in the two device fields
    if (out) memcpy(out, g_events_last.v, sizeof(g_events_last.v));
}

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
    if (!g_align_last.ws)
        return fail(DD_ERR_INVALID, "dd_hap_variants_device: no alignment launch of this thread to run behind (its workspace header holds the pair counter)");
    dda::VariantsArgs A;
    A.n_refs = b->n_refs; A.n_pairs = b->n_pairs;
    A.ref_off = b->ref_off; A.ref_seq = reinterpret_cast<const uint8_t *>(b->ref_seq);
    A.pair_ref = b->pair_ref; A.hap_off = b->hap_off; A.hap_seq = reinterpret_cast<const uint8_t *>(b->hap_seq);
    A.status = r->status; A.ref_pos = r->ref_pos;
    A.summary = summary; A.variants = variants; A.cap = cap;
    A.hdr = reinterpret_cast<unsigned int *>(const_cast<unsigned char *>(g_align_last.ws));
    const int64_t rec[DD_ALIGN_EVENTS_LOG_FIELDS] = {(int64_t)dda::variants_grid(b->n_pairs), (int64_t)b->n_pairs, -1, -1};
    memcpy(g_variants_last.v, rec, sizeof(rec));
    g_variants_last.ws = g_align_last.ws; g_variants_last.stream = static_cast<hipStream_t>(stream); g_variants_last.have_stats = false;
    HIP_TRY(dda::launch_hap_variants(A, static_cast<hipStream_t>(stream)));
    return DD_SUCCESS;
}

void dd_hap_variants_last_launch(int64_t out[DD_ALIGN_EVENTS_LOG_FIELDS])
{
    (void)read_variants_stats();               // a failure leaves -1 in the two device fields
    if (out) memcpy(out, g_variants_last.v, sizeof(g_variants_last.v));
}

} // extern "C"

namespace ddh {
namespace {

// the three host-pointer entries: ev = va = nullptr is dd_align_haplotypes; with events or variants the slice comes back only where the
// caller has room for it
struct EventsOut { int32_t *n_events; dd_align_events *events; int cap; };
struct VariantsOut { dd_hap_variants_summary *summary; dd_hap_variant *variants; int cap; };

int align_host_entry(const dd_align_batch *b, dd_align_result *r, const EventsOut *ev, int device, const VariantsOut *va = nullptr)
{
    AlignShape s;
    int rc = check_align_batch(b, s);
    if (rc) return rc;
    if (!r) return fail(DD_ERR_INVALID, "null align result");
    if (b->n_pairs > 0 && (!r->score || !r->status)) return fail(DD_ERR_INVALID, "null score or status in align result");
    if (!ev && !va && s.hap_bytes > 0 && !r->ref_pos) return fail(DD_ERR_INVALID, "null ref_pos in align result");
    if (va) {
        if (va->cap < 1 || va->cap > DD_HAP_VARIANTS_MAX_CAP) return fail(DD_ERR_INVALID, "cap outside 1 ... DD_HAP_VARIANTS_MAX_CAP");
        if (b->n_pairs > 0 && (!va->summary || !va->variants)) return fail(DD_ERR_INVALID, "null summary or variants");
    }
    if (ev) {
        if (ev->cap < 1 || ev->cap > DD_ALIGN_EVENTS_MAX_CAP) return fail(DD_ERR_INVALID, "events_cap outside 1 ... DD_ALIGN_EVENTS_MAX_CAP");
        if (b->n_pairs > 0 && (!ev->n_events || !ev->events)) return fail(DD_ERR_INVALID, "null n_events or events");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(DD_ERR_NO_DEVICE, "no HIP device: the haplotype alignment has no CPU fallback in this library");
    if (device < 0 || device >= ndev) return fail(DD_ERR_NO_DEVICE, "device ordinal out of range");
    HIP_TRY(hipSetDevice(device));
    if (b->n_pairs == 0) return DD_SUCCESS;

    // one allocation, 256-byte aligned pieces: offsets, sequences, outputs, workspace
    const size_t ws_bytes = dd_align_workspace_bytes(b);
    const size_t P = (size_t)b->n_pairs, R = (size_t)b->n_refs;
    const size_t ev_bytes = ev ? P * (size_t)ev->cap * sizeof(dd_align_events) : 0;
    const size_t va_bytes = va ? P * (size_t)va->cap * sizeof(dd_hap_variant) : 0;
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t o = off; off = (off + std::max<size_t>(bytes, 1) + 255u) & ~size_t(255u); return o; };
    const size_t o_roff = take((R + 1) * 4), o_rseq = take((size_t)s.ref_bytes), o_pref = take(P * 4), o_hoff = take((P + 1) * 4),
                 o_hseq = take((size_t)s.hap_bytes), o_score = take(P * 4), o_status = take(P * 4), o_rpos = take((size_t)s.hap_bytes * 2),
                 o_ws = take(ws_bytes), o_nev = take(ev ? P * 4 : 0), o_ev = take(ev_bytes),
                 o_sum = take(va ? P * sizeof(dd_hap_variants_summary) : 0), o_va = take(va_bytes);
    struct Mem {
        unsigned char *p = nullptr;
        ~Mem() { if (p) (void)hipFree(p); }
    } mem;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&mem.p), off));
    unsigned char *d = mem.p;
    HIP_TRY(hipMemcpy(d + o_roff, b->ref_off, (R + 1) * 4, hipMemcpyHostToDevice));
    if (s.ref_bytes) HIP_TRY(hipMemcpy(d + o_rseq, b->ref_seq, (size_t)s.ref_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d + o_pref, b->pair_ref, P * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d + o_hoff, b->hap_off, (P + 1) * 4, hipMemcpyHostToDevice));
    if (s.hap_bytes) HIP_TRY(hipMemcpy(d + o_hseq, b->hap_seq, (size_t)s.hap_bytes, hipMemcpyHostToDevice));
    dd_align_batch db = *b;
    db.ref_off = reinterpret_cast<const int32_t *>(d + o_roff); db.ref_seq = reinterpret_cast<const char *>(d + o_rseq);
    db.pair_ref = reinterpret_cast<const int32_t *>(d + o_pref); db.hap_off = reinterpret_cast<const int32_t *>(d + o_hoff);
    db.hap_seq = reinterpret_cast<const char *>(d + o_hseq);
    const dd_align_result dr = {reinterpret_cast<int32_t *>(d + o_score), reinterpret_cast<int32_t *>(d + o_status),
                                reinterpret_cast<int16_t *>(d + o_rpos)};
    if ((rc = dd_align_haplotypes_device(&db, &dr, s.max_ref_len, s.max_hap_len, d + o_ws, ws_bytes, nullptr))) return rc;
    if (ev) {
        // records no event reaches stay 0: the caller's array is overwritten as a whole
        HIP_TRY(hipMemsetAsync(d + o_ev, 0, ev_bytes, nullptr));
        rc = dd_align_events_device(&db, &dr, reinterpret_cast<int32_t *>(d + o_nev), reinterpret_cast<dd_align_events *>(d + o_ev), ev->cap, nullptr);
        if (rc) { g_align_last.ws = nullptr; g_events_last.ws = nullptr; return rc; }
    }
    if (va) {
        // records no variant reaches stay 0: the caller's array is overwritten as a whole
        HIP_TRY(hipMemsetAsync(d + o_va, 0, va_bytes, nullptr));
        rc = dd_hap_variants_device(&db, &dr, reinterpret_cast<dd_hap_variants_summary *>(d + o_sum), reinterpret_cast<dd_hap_variant *>(d + o_va), va->cap, nullptr);
        if (rc) { g_align_last.ws = nullptr; g_variants_last.ws = nullptr; return rc; }
    }
    HIP_TRY(hipStreamSynchronize(nullptr));
    if ((rc = read_align_stats())) return rc;  // the workspace goes with this call
    g_align_last.ws = nullptr;
    if (va) {
        if ((rc = read_variants_stats())) return rc;
        g_variants_last.ws = nullptr;
    }
    if (ev) {
        if ((rc = read_events_stats())) return rc;
        g_events_last.ws = nullptr;
    }
    HIP_TRY(hipMemcpy(r->score, dr.score, P * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(r->status, dr.status, P * 4, hipMemcpyDeviceToHost));
    if (s.hap_bytes && r->ref_pos) HIP_TRY(hipMemcpy(r->ref_pos, dr.ref_pos, (size_t)s.hap_bytes * 2, hipMemcpyDeviceToHost));
    if (ev) {
        HIP_TRY(hipMemcpy(ev->n_events, d + o_nev, P * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(ev->events, d + o_ev, ev_bytes, hipMemcpyDeviceToHost));
    }
    if (va) {
        HIP_TRY(hipMemcpy(va->summary, d + o_sum, P * sizeof(dd_hap_variants_summary), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(va->variants, d + o_va, va_bytes, hipMemcpyDeviceToHost));
    }
    return DD_SUCCESS;
}

} // namespace
} // namespace ddh

extern "C" {

int dd_align_haplotypes(const dd_align_batch *b, dd_align_result *r, int device) { return align_host_entry(b, r, nullptr, device); }

int dd_align_haplotypes_events(const dd_align_batch *b, dd_align_result *r, int32_t *n_events, dd_align_events *events, int events_cap, int device)
{
    const EventsOut ev = {n_events, events, events_cap};
    return align_host_entry(b, r, &ev, device);
}

int dd_align_haplotypes_variants(const dd_align_batch *b, dd_align_result *r, dd_hap_variants_summary *summary, dd_hap_variant *variants, int cap, int device)
{
    const ddh::VariantsOut va = {summary, variants, cap};
    return align_host_entry(b, r, nullptr, device, &va);
}

} // extern "C"
