// host_path.cpp — the host-pointer entry points of the C ABI: the per-thread device arena and stream cache; one call as a sequence of stages
// (HostCall: check and screen, plan, list the inputs and outputs, reserve what the lists add up to, upload, cut window blocks, enqueue and
// collect chunked and double-buffered, drain on error); and the front end for several devices of one process.
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include "capi_internal.h"
#include "diploid_pair_kernel.h"

namespace ddh {
namespace {
// Per-host-thread cache kept between calls of the host-pointer entry points: one device arena, a pinned host
// mirror for small batches and two streams.  The literal drop-in use (one window per call) is dominated by
// allocation / copy-call overheads otherwise (1.5 ms per call with ~30 hipMalloc + ~35 hipMemcpy).
struct DeviceCtx {
    int device = -1;
    unsigned char *arena = nullptr;  size_t arena_cap = 0;
    unsigned char *pinned = nullptr; size_t pinned_cap = 0;
    hipStream_t s[2] = {nullptr, nullptr};
    void release()
    {
        if (device < 0) return;
        (void)hipSetDevice(device);
        if (arena) (void)hipFree(arena);
        if (pinned) (void)hipHostFree(pinned);
        for (int i = 0; i < 2; i++) if (s[i]) (void)hipStreamDestroy(s[i]);
        arena = pinned = nullptr; arena_cap = pinned_cap = 0; s[0] = s[1] = nullptr; device = -1;
    }
    int reserve(int dev, size_t dev_bytes, size_t pinned_bytes)
    {
        if (device != dev) { release(); device = dev; }
        hipError_t e;
        if (dev_bytes > arena_cap) {
            if (arena) (void)hipFree(arena);
            arena = nullptr; arena_cap = 0;
            const size_t want = dev_bytes + dev_bytes / 8 + (1u << 20);
            void *p = nullptr;
            if ((e = hipMalloc(&p, want)) != hipSuccess) return fail(DD_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
            arena = static_cast<unsigned char *>(p); arena_cap = want;
        }
        if (pinned_bytes > pinned_cap) {
            if (pinned) (void)hipHostFree(pinned);
            pinned = nullptr; pinned_cap = 0;
            const size_t want = pinned_bytes + pinned_bytes / 4 + (1u << 16);
            void *p = nullptr;
            if ((e = hipHostMalloc(&p, want, hipHostMallocDefault)) != hipSuccess) return fail(DD_ERR_HIP, std::string("hipHostMalloc: ") + hipGetErrorString(e));
            pinned = static_cast<unsigned char *>(p); pinned_cap = want;
        }
        for (int i = 0; i < 2; i++)
            if (!s[i] && (e = hipStreamCreateWithFlags(&s[i], hipStreamNonBlocking)) != hipSuccess)
                return fail(DD_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
        return DD_SUCCESS;
    }
};
// A host thread that ends gives its arena, pinned mirror and streams back (short-lived worker threads would otherwise
// leak them without bound).  Once exit() has begun the HIP runtime may already be unloading: then the cache is left to the
// process teardown.  The flag is raised by an atexit handler registered when the first cache is created, i.e. after the HIP
// runtime registered its own, so it runs before them.
std::atomic<bool> g_process_exiting(false);
void note_process_exit() { g_process_exiting.store(true); }
struct CtxHolder {
    DeviceCtx c;
    CtxHolder() { static const int once = atexit(note_process_exit); (void)once; }
    ~CtxHolder() { if (!g_process_exiting.load()) c.release(); }
};
thread_local CtxHolder g_ctx;

// Bump allocator over the cached arena.  In `staged` mode uploads are memcpy'd into the pinned mirror at the same
// offsets and shipped with ONE hipMemcpyAsync (flush_uploads); otherwise each upload is its own (large) copy.
struct DevBuf {
    DeviceCtx &C;
    size_t used = 0;
    bool staged = false;
    explicit DevBuf(DeviceCtx &c) : C(c) {}
    static size_t align(size_t v) { return (v + 255u) & ~size_t(255u); }
    // where an array of `bytes` placed behind `at` ends: alloc's own arithmetic, for a caller that adds up what it is going to place
    static size_t end_of(size_t at, size_t bytes) { return align(at) + (bytes ? bytes : 1); }
    template <class T> int alloc(T **out, size_t n)
    {
        const size_t end = end_of(used, n * sizeof(T));
        if (end > C.arena_cap) return fail(DD_ERR_HIP, "internal: device arena under-sized");   // (of last resort: callers reserve what they place)
        *out = reinterpret_cast<T *>(C.arena + align(used));
        used = end;
        return DD_SUCCESS;
    }
    template <class T> int upload(const T **out, const T *src, size_t n)
    {
        T *d = nullptr;
        int rc = alloc(&d, n);
        if (rc) return rc;
        if (n) {
            if (staged) {
                memcpy(C.pinned + (reinterpret_cast<unsigned char *>(d) - C.arena), src, n * sizeof(T));
            } else {
                hipError_t e = hipMemcpy(d, src, n * sizeof(T), hipMemcpyHostToDevice);
                if (e != hipSuccess) return fail(DD_ERR_HIP, std::string("hipMemcpy H2D: ") + hipGetErrorString(e));
            }
        }
        *out = d;
        return DD_SUCCESS;
    }
    int flush_uploads(hipStream_t st)
    {
        if (!staged || !used) return DD_SUCCESS;
        hipError_t e = hipMemcpyAsync(C.arena, C.pinned, used, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return fail(DD_ERR_HIP, std::string("hipMemcpyAsync H2D: ") + hipGetErrorString(e));
        return DD_SUCCESS;
    }
};

thread_local int g_last_direct = 0;     // output arrays the last host-pointer call on this thread let the kernels write in place

// The device address of [host, host + bytes) if that is page-locked host memory this device can address (dd_host_alloc, hipHostMalloc)
// and its last byte belongs to the same registered range; else NULL.
void *mapped_device_ptr(const void *host, size_t bytes)
{
    if (!host || !bytes) return nullptr;
    hipPointerAttribute_t a, e;
    if (hipPointerGetAttributes(&a, host) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (a.type != hipMemoryTypeHost || !a.devicePointer) return nullptr;
    if (hipPointerGetAttributes(&e, static_cast<const unsigned char *>(host) + bytes - 1) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (e.type != hipMemoryTypeHost || !e.devicePointer ||
        static_cast<unsigned char *>(e.devicePointer) - static_cast<unsigned char *>(a.devicePointer) != (ptrdiff_t)(bytes - 1)) return nullptr;
    return a.devicePointer;
}

// Where window w starts in each index space of dd_result (DD_RESULT_FIELDS); at(space, n_windows) is the space's length.
struct ResultIndex {
    const int64_t *pair_off, *hpos_off, *varcov_off;   // dd_batch_offsets
    const int32_t *read_off;                            // the batch's win_read_off
    int64_t at(ResultSpace s, int w) const
    {
        return s == SPACE_PAIR ? pair_off[w] : s == SPACE_HPOS ? hpos_off[w] : s == SPACE_VARCOV ? varcov_off[w] : s == SPACE_WINDOW ? w : read_off[w];
    }
};

// What a host-pointer call checks first; sz: the batch's sizes.  A batch without pairs (sz.n_pairs == 0) is finished here.
int front_checks(const dd_params *p, const dd_batch *b, dd_result *r, dd_sizes &sz, uint32_t options = 0)
{
    int rc = check_params(p, options);
    if (rc) return rc;
    if (!r || !r->ll || !r->status) return fail(DD_ERR_INVALID, "ll and status outputs are required");
    if ((rc = dd_batch_sizes(b, &sz))) return rc;
    // reads without haplotypes: no pair, but onHap[r] is an output per READ (the onHap kernel writes 0 there)
    if (sz.n_pairs == 0 && r->onHap && sz.n_reads > 0) memset(r->onHap, 0, (size_t)sz.n_reads * sizeof(*r->onHap));
    return DD_SUCCESS;
}

// true iff some p[i] >= limit.  The arrays checked this way hold one byte per read base (2e8 for configs[1]): a branch-free
// pass the compiler vectorises, cut into pieces for a few threads when it is long.
bool any_at_or_above(const uint8_t *p, size_t n, unsigned limit)
{
    if (limit > 255 || n == 0) return false;
    auto scan = [p, limit](size_t lo, size_t hi) -> unsigned {
        unsigned bad = 0;
        for (size_t i = lo; i < hi; i++) bad |= (unsigned)(p[i] >= limit);
        return bad;
    };
    const size_t piece = (size_t)8 << 20;
    unsigned hw = std::thread::hardware_concurrency();
    size_t nt = std::min<size_t>(std::min<size_t>(8, hw ? hw : 1), (n + piece - 1) / piece);
    if (nt <= 1) return scan(0, n) != 0;
    std::vector<unsigned> bad(nt, 0);
    std::vector<std::thread> th;
    for (size_t t = 1; t < nt; t++) th.emplace_back([&, t]() { bad[t] = scan(n * t / nt, n * (t + 1) / nt); });
    bad[0] = scan(0, n / nt);
    for (auto &x : th) x.join();
    for (size_t t = 0; t < nt; t++) if (bad[t]) return true;
    return false;
}

// DD_TIMING=1: where a host-pointer call spends its time outside the kernels (stderr, one line per call)
struct StageClock {
    bool on; std::chrono::steady_clock::time_point t; std::string line;
    StageClock() : on(getenv("DD_TIMING") != nullptr), t(std::chrono::steady_clock::now()) {}
    void mark(const char *what)
    {
        if (!on) return;
        const std::chrono::steady_clock::time_point n = std::chrono::steady_clock::now();
        char buf[64];
        snprintf(buf, sizeof(buf), " %s=%.2fms", what, std::chrono::duration<double, std::milli>(n - t).count());
        line += buf;
        t = n;
    }
    ~StageClock() { if (on) fprintf(stderr, "dd_timing:%s\n", line.c_str()); }
};

// One output array of a call: a field of dd_result, dd_cigar_result or dd_realign_result.  Placement in the arena, the in-place decision, the
// per-block download and the staged copy-back are written once, over the call's list of these.
struct OutArray {
    void *host;                  // the caller's array: part of the copy back (NULL: not asked for)
    size_t elem;                 // bytes per element
    ResultSpace space;           // its index space
    size_t width;                // elements per index (ops: ops_cap)
    bool in_place;               // page-locked caller memory is written by the kernels themselves
    bool device_only;            // no caller array, yet a kernel of this call reads it: placed behind the copy-back region, never copied
    ArenaSlot slot;              // its bytes, and the field of the device-side struct that takes its address
    unsigned char *dev = nullptr;
    bool direct = false;         // placement found `host` page-locked and device-addressable: dev is its device address
    bool copied_back() const { return host && !direct; }
};
#define OUT_INDEX(f, space, in_place) OUT_##f,
enum { DD_RESULT_FIELDS(OUT_INDEX) N_RESULT_OUTS };    // a dd_result field's place in the list
#undef OUT_INDEX

// What a CIGAR or realign entry adds to a call: inputs of its own, per window block one launch behind the likelihood launches, and output
// arrays in one index space (per PAIR: dd_compute_likelihoods_cigars; per READ: dd_compute_likelihoods_realign, which takes the window pairs
// and indel counts of its PAIR mode besides; dd_compute_likelihoods_realign_diploid, whose window pairs are chosen by a launch of its own in
// front of the realign launch and stay on the device, with outputs per WINDOW besides).  A key request (dd_compute_likelihoods_faster_keys,
// the --faster model) has no input of its own and one output per PAIR, the indel-map key count.
struct ExtraRequest {
    const int32_t *hap_ref_pos; const uint8_t *hap_aligned; int ops_cap;
    bool realign;
    dd_cigar_result cigars;                                                       // !realign
    int mode; const int32_t *win_hap_pair, *hap_n_indels; dd_realign_result reads; // realign
    bool diploid; const double *prior; dd_diploid_pair_result pairs;              // realign in PAIR mode, the pairs from dd_diploid_pairs_device
    int16_t *keys;                                                                // non-NULL: a key request, and nothing of the above
    // An audit request (dd_compute_likelihoods_audit, the main model) has nothing of the above either: a sample of the batch's windows, chosen
    // once, is recomputed per window block by the long-window kernel into a shadow as large as the sample and compared on the device with the
    // block's results; one report for the call comes back.  With the --faster model (dd_compute_likelihoods_faster_audit) the sample is that
    // model's (dd_audit_select_faster), the recomputation the shadow kernel's (faster_shadow_kernel.hip), and a key request may ride along.
    bool audit; uint64_t audit_seed; int32_t audit_want; void *audit_report; int64_t audit_max_records;
};

// test hook (dd_audit_inject_next): the window whose first pair's ll has one bit inverted in front of this thread's next audit, -1 = none
thread_local int g_audit_inject = -1;

// One call of a host-pointer entry.  run() is the sequence of its stages; the members are grouped by the stage that fills them.
struct HostCall {
    const Model model; const dd_params *const p; const dd_batch *const b; dd_result *const r; const int device; const uint32_t options;
    const ExtraRequest *const x;
    StageClock clk;
    dd_sizes sz;
    // check_and_screen
    std::vector<uint8_t> win_skip;
    uint8_t sym_lut[256];
    int n_skip = 0;
    bool long_on = false;
    bool wide_main = false;                              // main model, DD_OPT_WIDE_DELETIONS and maxLengthDel > 31: the long path's wide launch is the only one
    LongPath *long_path = nullptr;                       // the model's long path (used only if long_on)
    int32_t long_max[4] = {0, 0, 0, 0};
    std::vector<double> lib_logprob, lib_log95;
    // plan
    int W = 0;
    std::vector<int32_t> hap_window, class_list;
    std::vector<int64_t> pair_off, hpos_off, vc_off, hh_off;   // hh_off: dd_pair_sum_offsets (a diploid request's prior table)
    std::vector<double> tables;
    ResultIndex idx;
    dd_length_classes lcls = {};
    bool single_class = true;
    dd_device_batch db = {};
    size_t ws_bytes = 0, lws_bytes = 0;                  // per stream: the main kernels' workspace, the long path's own
    // describe: the three lists, and the device-side variables their slots fill
    std::vector<ArenaSlot> ins, scratch;
    std::vector<OutArray> outs;
    const int32_t *class_list_dev = nullptr, *hap_ref_pos_dev = nullptr, *win_hap_pair_dev = nullptr, *hap_n_indels_dev = nullptr;
    const uint8_t *hap_aligned_dev = nullptr;
    dd_result dr = {};
    dd_cigar_result dcg = {};
    dd_realign_result drl = {};
    dd_diploid_pair_result ddp = {};
    const double *prior_dev = nullptr;
    const int64_t *hh_off_dev = nullptr;
    int16_t *keys_dev = nullptr;
    // an audit request: the sample (plan), its device copies, the shadow, the report, per stream a workspace, per block two stats words
    std::vector<uint8_t> audit_class;
    std::vector<int64_t> au_pair_off, au_hpos_off, au_vc_off;
    dd_audit_view au_view = {};                          // device addresses once the inputs are placed
    bool audit_on = false;
    size_t aws_bytes = 0;
    dd_result shadow = {};
    unsigned char *report_dev = nullptr, *aws[2] = {nullptr, nullptr};
    unsigned long long *audit_stats = nullptr;
    int inject_window = -1;
    double inject_ll[2] = {0.0, 0.0};                    // the value as it was, and with its lowest bit inverted
    unsigned char *ws[2] = {nullptr, nullptr}, *lws[2] = {nullptr, nullptr};
    unsigned long long *long_stats = nullptr;           // long_path->n_stats (2 or 4) words per window block's long launch
    // reserve_and_upload, place_outputs
    DeviceCtx &ctx = g_ctx.c;
    DevBuf dev{ctx};
    bool staged = false, late_reads = false;
    size_t out_begin = 0, out_end = 0;                   // the copy-back region of the arena
    // cut_blocks
    std::vector<int> cw;                                 // window boundaries of the blocks
    int n_chunks = 1;


    int run()
    {
        launch_log_clear();
        g_long.log.clear();
        g_flong.log.clear();
        int rc = front_checks(p, b, r, sz, options);
        if (!rc && sz.n_pairs == 0 && x && x->realign)       // reads without haplotypes: no pair, nothing to launch, every read marked
            for (int64_t q = 0; q < sz.n_reads; q++) {
                const dd_realign_result &o = x->reads;
                o.hap[q] = -1; o.status[q] = DD_REALIGN_NO_HAPS; o.n_ops[q] = 0; o.ref_off[q] = -1;
            }
        if (!rc && sz.n_pairs == 0 && x && x->diploid)       // ... and no likelihood: the windows' pairs from the priors alone, by the CPU evaluation
            rc = dd_diploid_pairs_host(b, nullptr, nullptr, x->prior, &x->pairs, 1);
        if (rc || sz.n_pairs == 0) return rc;
        if ((rc = check_and_screen())) return rc;
        if ((rc = use_device(device, "no HIP device: the likelihood path has no CPU fallback"))) return rc;
        if ((rc = plan())) return rc;
        describe();
        if ((rc = reserve_and_upload())) return rc;
        if ((rc = place_outputs())) return rc;
        cut_blocks();
        clk.mark("outputs");
        rc = enqueue_and_collect();
        clk.mark("run");
        if (rc != DD_SUCCESS) {
            // kernels / copies already enqueued keep writing into the caller's buffers and this thread's arena: drain both
            // streams before the error is reported, so that neither is reused while still in flight
            const std::string msg = g_err;
            (void)hipStreamSynchronize(ctx.s[0]);
            (void)hipStreamSynchronize(ctx.s[1]);
            g_err = msg;
        }
        return rc;
    }

    // ---- the batch's content, and which windows the kernels cover (no HIP call) ----
    int check_and_screen()
    {
        int rc;
        if (!b->hap_seq || !b->read_seq || !b->read_qidx || !b->read_mqidx || !b->read_start || !b->read_flags ||
            !b->win_hap_start || !b->qual_table || !b->mapq_table)
            return fail(DD_ERR_INVALID, "null input array");
        if (b->n_qual < 1 || b->n_qual > DD_MAX_QUAL_TABLE || b->n_mapq < 1 || b->n_mapq > DD_MAX_QUAL_TABLE)
            return fail(DD_ERR_INVALID, "quality tables must hold 1..256 entries");
        // windows whose shape the kernels do not cover are skipped one by one (DD_PAIR_UNSUPPORTED), not the batch
        win_skip.resize((size_t)b->n_windows);
        int32_t ok_max[2] = {0, 0};
        if (!b->hap_seq_off || !b->read_seq_off) return fail(DD_ERR_INVALID, "null offset array");
        const int sym_left = assign_symbols(b, sym_lut);     // > 0: more than 26 distinct non-ACGTN haplotype bytes in the batch
        if (sym_left < 0) return sym_left;
        clk.mark("symbols");
        // long windows (DD_OPT_LONG_WINDOWS): win_skip holds the classes; the main kernels skip both non-zero classes, the long launch that
        // follows each block's main launches computes class 2
        // (DD_OPT_LONG_WINDOWS_FASTER: the same for the --faster model, with its own classes and its own kernel)
        const bool fl_on = model == MODEL_S && (options & DD_OPT_LONG_WINDOWS_FASTER);
        long_on = (model == MODEL_FBMAXERR && (options & DD_OPT_LONG_WINDOWS)) || fl_on;
        long_path = fl_on ? &g_flong : &g_long;
        wide_main = model == MODEL_FBMAXERR && long_on && wide_on(p, options);
        if (long_on) {
            n_skip = screen_windows_ex(p, b, options, win_skip.data(), long_max, sym_lut, sym_left > 0);
            ok_max[0] = long_max[0]; ok_max[1] = long_max[1];
            for (int w = 0; w < b->n_windows; w++) if (win_skip[(size_t)w] == DD_WIN_LONG) n_skip++;   // (counts every window the main kernels skip)
        } else {
            n_skip = screen_windows(b, win_skip.data(), ok_max, sym_lut, sym_left > 0 && model == MODEL_FBMAXERR);
        }
        sz.max_hap_len = ok_max[0] > 0 ? ok_max[0] : 1;      // planning maxima: the windows that are computed
        sz.max_read_len = ok_max[1] > 0 ? ok_max[1] : 1;
        clk.mark("screen");
        if (p->mapUnmappedReads && model == MODEL_FBMAXERR) {
            if (!b->read_mate_pos || !b->read_mate_len || !b->read_lib)
                return fail(DD_ERR_INVALID, "mapUnmappedReads needs read_mate_pos, read_mate_len and read_lib");
            if (b->n_libs < 1 || !b->lib_off) return fail(DD_ERR_INVALID, "mapUnmappedReads needs the library tables");
            lib_logprob.resize((size_t)(b->lib_off[b->n_libs] > 0 ? b->lib_off[b->n_libs] : 1));
            lib_log95.resize((size_t)b->n_libs);
            if ((rc = dd_build_library_tables(b, lib_logprob.data(), lib_log95.data()))) return rc;
            for (int64_t q = 0; q < sz.n_reads; q++)
                if (b->read_lib[q] >= b->n_libs) return fail(DD_ERR_INVALID, "read_lib out of range");
        }
        if (any_at_or_above(b->read_mqidx, (size_t)sz.n_reads, (unsigned)b->n_mapq)) return fail(DD_ERR_INVALID, "read_mqidx out of range");
        if (any_at_or_above(b->read_qidx, (size_t)sz.read_bases, (unsigned)b->n_qual)) return fail(DD_ERR_INVALID, "read_qidx out of range");
        for (int i = 0; i < b->n_qual; i++)
            if (!(b->qual_table[i] >= 0.0 && b->qual_table[i] <= 1.0)) return fail(DD_ERR_INVALID, "base quality outside [0,1]");
        for (int i = 0; i < b->n_mapq; i++)
            if (!(b->mapq_table[i] >= 0.0 && b->mapq_table[i] < 1.0)) return fail(DD_ERR_INVALID, "mapping quality outside [0,1)");
        clk.mark("validate");
        return DD_SUCCESS;
    }

    // ---- host-side planning (no device work yet): index, tables, launch classes and workspace sizes ----
    int plan()
    {
        int rc;
        W = b->n_windows;
        hap_window.resize((size_t)sz.n_haps);
        pair_off.resize(W + 1); hpos_off.resize(W + 1); vc_off.resize(W + 1);
        dd_build_index(b, hap_window.data(), pair_off.data(), hpos_off.data(), vc_off.data());
        idx = {pair_off.data(), hpos_off.data(), vc_off.data(), b->win_read_off};
        if (x && x->diploid) {
            hh_off.resize(W + 1);
            if ((rc = dd_pair_sum_offsets(b, hh_off.data()))) return rc;
        }
        tables.resize(DD_TABLE_DOUBLES);
        rc = build_tables(p, b->qual_table, b->n_qual, b->mapq_table, b->n_mapq, tables.data(), options);
        if (rc < 0) return rc;
        // Ragged batches: one launch per (lane tiling of the haplotypes, read-length interval) that has work (build_launch_classes) — a single
        // 170-bp haplotype or 250-bp read does not drag every pair of the batch onto the K = 3 / long-read build.
        if (model == MODEL_FBMAXERR && !wide_main && !getenv("DD_NO_LENGTH_CLASSES")) {          // env: A/B only
            class_list.resize((size_t)sz.n_haps * DD_N_READ_CLASSES + 1);
            if ((rc = build_launch_classes(b, n_skip ? win_skip.data() : nullptr, p, class_list.data(), &lcls))) return rc;
        }
        db.n_windows = W; db.n_haps = (int32_t)sz.n_haps; db.n_reads = (int32_t)sz.n_reads;
        db.max_hap_len = sz.max_hap_len; db.max_read_len = sz.max_read_len;
        db.n_qual = b->n_qual; db.n_mapq = b->n_mapq;
        for (int w = 0; w < W; w++)
            if (!win_skip[(size_t)w] && b->win_read_off[w + 1] - b->win_read_off[w] > db.max_window_reads) db.max_window_reads = b->win_read_off[w + 1] - b->win_read_off[w];
        ws_bytes = (model == MODEL_S || wide_main) ? 0 : dd_workspace_bytes(p, &db);
        single_class = lcls.n_launches <= 1;
        if (!single_class) {
            db.classes = &lcls;
            db.hap_class_list = class_list.data();             // (host pointer: only dd_workspace_bytes' class walk looks at it here)
            const size_t w2 = dd_workspace_bytes(p, &db);
            if (w2 > ws_bytes) ws_bytes = w2;
            db.classes = nullptr; db.hap_class_list = nullptr;
        }
        if (x && x->audit) {
            // the sample, once for the whole batch; every window block audits its own chosen windows
            audit_class.resize((size_t)std::max(W, 1)); au_pair_off.resize(W + 1); au_hpos_off.resize(W + 1); au_vc_off.resize(W + 1);
            const uint8_t *cls = n_skip ? win_skip.data() : nullptr;
            rc = model == MODEL_S ? dd_audit_select_faster(p, b, cls, options & DD_OPT_LONG_WINDOWS_FASTER, x->audit_seed, x->audit_want, audit_class.data(),
                                                           au_pair_off.data(), au_hpos_off.data(), au_vc_off.data(), &au_view.sizes)
                                  : dd_audit_select(p, b, cls, x->audit_seed, x->audit_want, audit_class.data(), au_pair_off.data(),
                                                    au_hpos_off.data(), au_vc_off.data(), &au_view.sizes);
            if (rc < 0) return rc;
            au_view.n_windows = W; au_view.n_qual = b->n_qual;
            audit_on = au_view.sizes.n_pairs > 0;
            if (audit_on && model == MODEL_S) {
                aws_bytes = std::max<size_t>(dd_audit_workspace_bytes_faster(p, &au_view), 256);    // (0: the shadow kernel's areas are in LDS)
            } else if (audit_on) {
                aws_bytes = dd_audit_workspace_bytes(p, &au_view);
                if (!aws_bytes) return fail(DD_ERR_UNSUPPORTED, "audit: no long-window plan for the sample's shape");
            }
            inject_window = g_audit_inject;
            g_audit_inject = -1;
        }
        if (long_on && long_max[2] > 0) {
            db.long_max_hap_len = long_max[2]; db.long_max_read_len = long_max[3];
            lws_bytes = wide_main ? dd_workspace_bytes_wide(p, &db) : long_path->workspace_bytes(p, &db);   // (the --faster long workspace does not depend on the parameters)
            if (!lws_bytes) return fail(DD_ERR_UNSUPPORTED, "long path: no plan for this shape");
        }
        clk.mark("plan");
        return DD_SUCCESS;
    }

    // ---- every array the call places in the arena, in the arena's order: inputs (the order of their copies), outputs, scratch ----
    template <class T> void in(const T **var, const T *src, size_t n, bool read_bases = false) { ins.push_back(arena_slot(var, n * sizeof(T), src, read_bases)); }
    template <class T> void out(T *host, T **dev_field, ResultSpace space, size_t width, bool in_place)
    {
        outs.push_back({host, sizeof(T), space, width, in_place, false, arena_slot(dev_field, (size_t)idx.at(space, W) * width * sizeof(T))});
    }
    void describe()
    {
        const size_t n_haps = (size_t)sz.n_haps, n_reads = (size_t)sz.n_reads;
        const size_t n_var = b->hap_var_off ? (size_t)b->hap_var_off[sz.n_haps] : 0;
        ins.reserve(40);
#define IN(field, n) in(&db.field, b->field, (size_t)(n))
        IN(win_hap_off, W + 1); IN(win_read_off, W + 1); IN(win_hap_start, W);
        IN(hap_seq_off, n_haps + 1); IN(hap_seq, sz.hap_bases);
        IN(read_seq_off, n_reads + 1);
        in(&db.read_seq, b->read_seq, (size_t)sz.read_bases, true);
        in(&db.read_qidx, b->read_qidx, (size_t)sz.read_bases, true);
        IN(read_mqidx, n_reads); IN(read_start, n_reads); IN(read_flags, n_reads);
        if (b->hap_var_off) {
            IN(hap_var_off, n_haps + 1); IN(hap_var, 2 * n_var);
            if (b->hap_var_flank) IN(hap_var_flank, 3 * n_var);
        }
        in(&db.hap_window, hap_window.data(), hap_window.size());
        in(&db.win_pair_off, pair_off.data(), pair_off.size());
        in(&db.win_hpos_off, hpos_off.data(), hpos_off.size());
        in(&db.win_varcov_off, vc_off.data(), vc_off.size());
        in(&db.tables, tables.data(), tables.size());
        in(&db.sym_lut, sym_lut, (size_t)256);
        if (n_skip > 0) in(&db.win_skip, win_skip.data(), win_skip.size());
        if (!lib_log95.empty()) {
            IN(read_mate_pos, n_reads); IN(read_mate_len, n_reads); IN(read_lib, n_reads); IN(lib_off, b->n_libs + 1);
            in(&db.lib_logprob, lib_logprob.data(), lib_logprob.size());
            in(&db.lib_log95, lib_log95.data(), lib_log95.size());
        }
#undef IN
        if (!single_class) in(&class_list_dev, class_list.data(), (size_t)lcls.list_len);
        if (audit_on) {
            in(&au_view.audit_class, audit_class.data(), audit_class.size());
            in(&au_view.pair_off, au_pair_off.data(), au_pair_off.size());
            in(&au_view.hpos_off, au_hpos_off.data(), au_hpos_off.size());
            in(&au_view.varcov_off, au_vc_off.data(), au_vc_off.size());
        }
        if (x && !x->keys && !x->audit) {
            in(&hap_ref_pos_dev, x->hap_ref_pos, (size_t)sz.hap_bases);
            if (x->hap_aligned) in(&hap_aligned_dev, x->hap_aligned, n_haps);
            if (x->realign && x->mode == DD_REALIGN_PAIR) {
                if (!x->diploid) in(&win_hap_pair_dev, x->win_hap_pair, (size_t)W * 2);
                in(&hap_n_indels_dev, x->hap_n_indels, n_haps);
            }
            if (x->diploid) {
                in(&hh_off_dev, hh_off.data(), hh_off.size());
                in(&prior_dev, x->prior, (size_t)hh_off[(size_t)W]);
            }
        }

        // Outputs: the fields of dd_result, then the request's own.  Output arrays the caller keeps in page-locked host memory that this device
        // can address (dd_host_alloc, hipHostMalloc) are written by the kernels themselves, over the link, as the pairs finish: no staging
        // copy in HBM and no copy afterwards.  (The runtime carries device -> host copies of this size out with a copy KERNEL:
        // profiles/r02/hostapi_timeline.txt shows 300 ms of such kernels on the CUs beside 410 ms of HMM kernels for configs[1].)  status and
        // offHapHMQ stay in HBM: the onHap kernel reads them back (DD_RESULT_FIELDS).
        outs.reserve(N_RESULT_OUTS + 10);
#define OUT(f, space, in_place) out(r->f, &dr.f, SPACE_##space, 1, in_place != 0);
        DD_RESULT_FIELDS(OUT)
#undef OUT
        if (r->onHap && !r->offHapHMQ) outs[OUT_offHapHMQ].device_only = true;    // onHap is derived from it
        if (x && x->audit) {
            // The comparison reads every result array on the device: arrays the caller keeps in page-locked memory are staged in HBM and copied
            // back like pageable ones, instead of being read back over the link.  An array the caller does not ask for is not compared.
            for (int i = 0; i < N_RESULT_OUTS; i++) outs[(size_t)i].in_place = false;
            if (x->keys) {                                   // the key launch reads hpos on the device, wanted back or not: it is compared then
                outs[OUT_hpos].device_only = !r->hpos;
                out(x->keys, &keys_dev, SPACE_PAIR, 1, false);
            }
        } else if (x) {
            // The request's launch reads hpos on the device: alignments the caller wants in page-locked memory are staged in HBM and copied back
            // like pageable ones, instead of being read back over the link; and they are needed there even when the caller does not want them
            // back (r->hpos == NULL: nothing of them is copied).  A realign launch reads ll and onHap on the device as well.
            outs[OUT_hpos].in_place = false;
            outs[OUT_hpos].device_only = !r->hpos;
            const size_t cap = (size_t)x->ops_cap;
            if (x->keys) out(x->keys, &keys_dev, SPACE_PAIR, 1, false);
#define OUT_PAIR(f, wide) out(x->cigars.f, &dcg.f, SPACE_PAIR, wide ? cap : 1, false);
#define OUT_READ(f, wide) out(x->reads.f, &drl.f, SPACE_READ, wide ? cap : 1, false);
#define OUT_WINDOW(f, width) out(x->pairs.f, &ddp.f, SPACE_WINDOW, width, false);
            if (x->realign) {
                outs[OUT_ll].in_place = outs[OUT_onHap].in_place = false;
                DD_REALIGN_FIELDS(OUT_READ)
                if (x->diploid) { DD_DIPPAIR_FIELDS(OUT_WINDOW) }
            } else if (!x->keys) {
                DD_CIGAR_FIELDS(OUT_PAIR)
            }
#undef OUT_PAIR
#undef OUT_READ
#undef OUT_WINDOW
        }

        for (int i = 0; i < 2; i++)
            if (ws_bytes) scratch.push_back(arena_slot(&ws[i], ws_bytes));
        if (lws_bytes) {
            for (int i = 0; i < 2; i++) scratch.push_back(arena_slot(&lws[i], lws_bytes));
            scratch.push_back(arena_slot(&long_stats, (size_t)4 * 64 * sizeof(*long_stats)));    // 64 blocks at most, 4 words at most
        }
        if (audit_on) {
            // the shadow: every array the comparison can use, as large as the sample; the caller sees none of it
            const dd_audit_sizes &as = au_view.sizes;
#define SHADOW(f, space, in_place)                                                                                                   \
            if (OUT_##f != OUT_onHap && dr_wanted(OUT_##f))                                                                               \
                scratch.push_back(arena_slot(&shadow.f, sizeof(*shadow.f) * (size_t)(SPACE_##space == SPACE_PAIR ? as.n_pairs : SPACE_##space == SPACE_HPOS ? as.hpos_len : as.var_cov_len)));
            DD_RESULT_FIELDS(SHADOW)
#undef SHADOW
            scratch.push_back(arena_slot(&report_dev, DD_AUDIT_REPORT_BYTES(x->audit_max_records)));
            for (int i = 0; i < 2; i++) scratch.push_back(arena_slot(&aws[i], aws_bytes));
            scratch.push_back(arena_slot(&audit_stats, (size_t)2 * 64 * sizeof(*audit_stats)));
        }
    }
    // an audit's shadow holds the arrays the call itself has on the device (the caller's, and offHapHMQ when onHap is derived from it)
    bool dr_wanted(int i) const { return outs[(size_t)i].host || outs[(size_t)i].device_only; }
    // where the arena ends once every array of the lists is placed behind `at`, in the order reserve_and_upload and place_outputs place them;
    // *copy_back_end: the end of the inputs and of the outputs that are copied back (what the pinned mirror of a staged call holds)
    size_t end_of_all(size_t at, size_t *copy_back_end) const
    {
        for (const ArenaSlot &s : ins) at = DevBuf::end_of(at, s.bytes);
        for (const OutArray &o : outs) if (o.host) at = DevBuf::end_of(at, o.slot.bytes);
        *copy_back_end = at;
        for (const OutArray &o : outs) if (o.device_only) at = DevBuf::end_of(at, o.slot.bytes);
        for (const ArenaSlot &s : scratch) at = DevBuf::end_of(at, s.bytes);
        return at;
    }

    // ---- the device arena (cached per host thread) and the inputs ----
    int reserve_and_upload()
    {
        int rc;
        size_t io_bytes = 0;
        const size_t arena_bytes = end_of_all(0, &io_bytes);
        // small batch: one H2D, one D2H through the pinned mirror.  Every input and every output asked for counts, also those that end up read
        // or written in place: what is page-locked is known only once the device is in use
        staged = io_bytes <= (size_t)64 << 20;
        if ((rc = ctx.reserve(device, arena_bytes, staged ? io_bytes : 0))) return rc;
        clk.mark("reserve");
        dev.staged = staged;
        // The two big inputs (one byte per read base each).  Large batches: only reserved here — each window block's share is copied
        // on the block's own stream right in front of its kernels, so all but the first block's transfer hides behind the kernels of
        // the block before.
        late_reads = !staged && sz.read_bases > 0;
        // Staged (small) batches whose two big inputs the caller keeps in page-locked, device-addressable memory (the C++ adapter packs
        // into dd_host_alloc buffers): the kernels read them in place over the link — each (read, haplotype) pair fetches its read once,
        // ~80 MB per 256-window batch at 8 haplotypes — instead of waiting for a staged copy whose blit kernels share the CUs with the
        // batch that is running (profiles/r03/window_loop_timeline.txt).  DD_ZERO_COPY_IN=0 switches it off (A/B).
        static const bool zero_copy_in = !(getenv("DD_ZERO_COPY_IN") && !strcmp(getenv("DD_ZERO_COPY_IN"), "0"));
        const void *ms = zero_copy_in && !late_reads ? mapped_device_ptr(b->read_seq, (size_t)sz.read_bases) : nullptr;
        const void *mq = zero_copy_in && !late_reads ? mapped_device_ptr(b->read_qidx, (size_t)sz.read_bases) : nullptr;
        for (const ArenaSlot &s : ins) {
            const unsigned char *d = nullptr;
            if (s.read_bases && ms && mq) d = static_cast<const unsigned char *>(s.var == &db.read_seq ? ms : mq);
            else if (s.read_bases && late_reads) rc = dev.alloc(const_cast<unsigned char **>(&d), s.bytes);
            else rc = dev.upload(&d, s.src, s.bytes);
            if (rc) return rc;
            s.point_at(d);
        }
        if ((rc = dev.flush_uploads(ctx.s[0]))) return rc;       // staged mode: the one H2D copy
        if (!staged) HIP_TRY(hipStreamSynchronize(nullptr));     // pageable uploads went through the null stream's DMA
        clk.mark("upload");
        return DD_SUCCESS;
    }

    // ---- outputs and scratch: which arrays the kernels write in place, the copy-back region, what lies behind it ----
    int place_outputs()
    {
        int rc;
        static const bool zero_copy_on = !(getenv("DD_ZERO_COPY") && !strcmp(getenv("DD_ZERO_COPY"), "0"));   // =0 switches in-place outputs off (A/B)
        int n_direct = 0;
        out_begin = DevBuf::align(dev.used);
        for (OutArray &o : outs) {
            if (!o.host) continue;
            void *m = (o.in_place && zero_copy_on) ? mapped_device_ptr(o.host, o.slot.bytes) : nullptr;
            if (m) { o.dev = static_cast<unsigned char *>(m); o.direct = true; n_direct++; }
            else if ((rc = dev.alloc(&o.dev, o.slot.bytes))) return rc;
        }
        out_end = dev.used;
        g_last_direct = n_direct;
        for (OutArray &o : outs)                                 // (behind the outputs: not part of the staged copy back)
            if (o.device_only && (rc = dev.alloc(&o.dev, o.slot.bytes))) return rc;
        for (const OutArray &o : outs) if (o.dev) o.slot.point_at(o.dev);
        for (const ArenaSlot &s : scratch) {
            unsigned char *d = nullptr;
            if ((rc = dev.alloc(&d, s.bytes))) return rc;
            s.point_at(d);
        }
        // DD_POISON_OUTPUTS (debug, read per call): every dd_result array placed in the arena starts out as bytes 0x5A instead of what the
        // thread's last call left at these offsets, so that an element no kernel of this call writes shows in the caller's copy.  Arrays
        // written in place are the caller's to fill; the CIGAR / realign / key arrays are left alone.  The window blocks alternate between
        // the two streams: the fill is complete before the first launch of either.
        if (getenv("DD_POISON_OUTPUTS")) {
            for (int i = 0; i < N_RESULT_OUTS; i++) {
                const OutArray &o = outs[(size_t)i];
                if (o.dev && !o.direct && o.slot.bytes) HIP_TRY(hipMemsetAsync(o.dev, 0x5A, o.slot.bytes, ctx.s[0]));
            }
            HIP_TRY(hipStreamSynchronize(ctx.s[0]));
        }
        return DD_SUCCESS;
    }

    // Chunked, double-buffered execution: contiguous window blocks alternate between two streams, and the D2H
    // of block c is issued after the kernel of block c+1 has been enqueued, so the copy engine drains results
    // while the CUs work on the next block (with pageable user memory the copy call blocks the host thread, not
    // the GPU).  Each stream has its own back-pointer scratch.  Small (staged) batches run as one block on stream 0
    // and come back with one D2H through the pinned mirror.
    void cut_blocks()
    {
        n_chunks = staged ? 1 : (int)((sz.n_pairs + 999999) / 1000000);
        if (n_chunks > 64) n_chunks = 64;
        if (n_chunks > W) n_chunks = W;
        if (n_chunks < 1) n_chunks = 1;
        cw.assign(n_chunks + 1, 0);                // window boundaries with ~equal pair counts
        for (int c = 1; c < n_chunks; c++) {
            const int64_t target = sz.n_pairs * c / n_chunks;
            int w = cw[c - 1];
            while (w < W && pair_off[w] < target) w++;
            cw[c] = w;
        }
        cw[n_chunks] = W;
    }

    // block c's share of every output that is copied back, on the block's stream
    int download(int c)
    {
        const int w0 = cw[c], w1 = cw[c + 1];
        for (const OutArray &o : outs) {
            const size_t off = (size_t)idx.at(o.space, w0) * o.width * o.elem, n = (size_t)idx.at(o.space, w1) * o.width * o.elem - off;
            if (o.copied_back() && n) HIP_TRY(hipMemcpyAsync(static_cast<unsigned char *>(o.host) + off, o.dev + off, n, hipMemcpyDeviceToHost, ctx.s[c & 1]));
        }
        return DD_SUCCESS;
    }

    // The request's launch for the windows [w0, w1) of a block, behind the block's likelihood launches on the same stream: the block's CIGARs
    // (its ops start out zero: a pair's unused slots are defined), or the block's realigned reads (reads of windows without haplotypes are
    // marked too: the launch goes by reads, not by pairs).  A diploid request's pair launch goes first, for the same windows: the realign
    // launch reads the pairs where that launch left them.  A key request: the block's counts.
    int launch_extra(hipStream_t st, int c, int w0, int w1)
    {
        int rc;
        if (x->keys && (rc = launch_indel_keys_range(&db, dr.hpos, dr.status, keys_dev, st, idx.at(SPACE_PAIR, w0), idx.at(SPACE_PAIR, w1)))) return rc;
        if (x->audit) return audit_on ? launch_audit_block(st, c, w0, w1) : DD_SUCCESS;
        if (x->keys) return DD_SUCCESS;
        if (x->diploid && (rc = launch_diploid_pairs_range(&db, hh_off_dev, dr.ll, dr.status, prior_dev, &ddp, st, w0, w1))) return rc;
        const ResultSpace space = x->realign ? SPACE_READ : SPACE_PAIR;
        const int64_t lo = idx.at(space, w0), hi = idx.at(space, w1);
        if (hi <= lo) return DD_SUCCESS;
        HIP_TRY(hipMemsetAsync((x->realign ? drl.ops : dcg.ops) + (size_t)lo * x->ops_cap, 0, (size_t)(hi - lo) * x->ops_cap * 4, st));
        if (!x->realign) return launch_cigars_range(&db, dr.hpos, dr.status, hap_ref_pos_dev, hap_aligned_dev, &dcg, x->ops_cap, st, lo, hi);
        const RealignInputs in = {x->mode, dr.ll, dr.onHap, x->diploid ? ddp.pair : win_hap_pair_dev, hap_n_indels_dev, dr.hpos, dr.status, hap_ref_pos_dev,
                                  hap_aligned_dev};
        return launch_realign_range(&db, in, &drl, x->ops_cap, st, (int)lo, (int)hi);
    }

    // An audit request's launches for the chosen windows of [w0, w1).  The test hook inverts the lowest bit of the device copy of ll of
    // window inject_window's first pair in front of them and puts the value back behind them: the audit sees it, the caller's results do not.
    int launch_audit_block(hipStream_t st, int c, int w0, int w1)
    {
        const int64_t j0 = au_pair_off[(size_t)w0], j1 = au_pair_off[(size_t)w1];
        if (j1 <= j0) return DD_SUCCESS;
        const bool inject = inject_window >= w0 && inject_window < w1 && pair_off[(size_t)inject_window + 1] > pair_off[(size_t)inject_window];
        double *target = inject ? dr.ll + pair_off[(size_t)inject_window] : nullptr;
        if (inject) {
            HIP_TRY(hipMemcpyAsync(&inject_ll[0], target, sizeof(double), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            uint64_t bits;
            memcpy(&bits, &inject_ll[0], sizeof(bits));
            bits ^= 1ull;
            memcpy(&inject_ll[1], &bits, sizeof(bits));
            HIP_TRY(hipMemcpyAsync(target, &inject_ll[1], sizeof(double), hipMemcpyHostToDevice, st));
        }
        const int rc = model == MODEL_S
                           ? launch_audit_faster_range(p, &db, &dr, &au_view, &shadow, report_dev, x->audit_max_records, aws[c & 1], st, j0, j1)
                           : launch_audit_range(p, &db, &dr, &au_view, &shadow, report_dev, x->audit_max_records, aws[c & 1], aws_bytes, st, w0, w1,
                                                b->win_read_off[w0], b->win_read_off[w1], j0, j1, audit_stats + 2 * c);
        if (inject) HIP_TRY(hipMemcpyAsync(target, &inject_ll[0], sizeof(double), hipMemcpyHostToDevice, st));     // also when the launch failed
        return rc;
    }

    int enqueue_and_collect()
    {
        int rc;
        if (audit_on) {                                      // one report for the call: zero before a block of either stream adds to it
            HIP_TRY(hipMemsetAsync(report_dev, 0, DD_AUDIT_REPORT_BYTES(x->audit_max_records), ctx.s[0]));     // the records too: unused slots come back zero
            HIP_TRY(hipStreamSynchronize(ctx.s[0]));
        }
        for (int c = 0; c < n_chunks; c++) {
            hipStream_t st = ctx.s[c & 1];
            const int w0 = cw[c], w1 = cw[c + 1];
            const int g0 = b->win_hap_off[w0], g1 = b->win_hap_off[w1], q0 = b->win_read_off[w0], q1 = b->win_read_off[w1];
            if (late_reads && q1 > q0) {
                const size_t s0 = (size_t)b->read_seq_off[q0], sn = (size_t)b->read_seq_off[q1] - s0;
                HIP_TRY(hipMemcpyAsync(const_cast<char *>(db.read_seq) + s0, b->read_seq + s0, sn, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(const_cast<uint8_t *>(db.read_qidx) + s0, b->read_qidx + s0, sn, hipMemcpyHostToDevice, st));
            }
            if (wide_main) {
                // no main-kernel build for these parameters: the wide launch below writes every pair of the block, placeholders included
            } else if (single_class) {
                if ((rc = launch_range(model, p, &db, &dr, ws[c & 1], ws_bytes, st, g0, g1, q0, q1, n_chunks > 1, nullptr, options))) return rc;
            } else {
                // every launch class of this window block, then onHap once
                for (int i = 0; i < lcls.n_launches; i++) {
                    const dd_launch_class &L = lcls.launch[i];
                    const int32_t *hl = class_list.data() + L.list_off;
                    LenClass lc = len_class_of(L, class_list_dev, i == lcls.n_launches - 1);
                    lc.list_begin = (int)(std::lower_bound(hl, hl + L.list_len, g0) - hl);
                    lc.list_end = (int)(std::lower_bound(hl, hl + L.list_len, g1) - hl);
                    if ((rc = launch_range(model, p, &db, &dr, ws[c & 1], ws_bytes, st, g0, g1, q0, q1, n_chunks > 1, &lc))) return rc;
                }
            }
            if (lws_bytes || wide_main) {
                bool any = wide_main;
                for (int w = w0; w < w1 && !any; w++) any = win_skip[(size_t)w] == DD_WIN_LONG;
                if (any && (rc = long_path->launch_range(p, &db, &dr, lws[c & 1], lws_bytes, st, w0, w1, q0, q1,
                                                         long_stats ? long_stats + long_path->n_stats * c : nullptr, options))) return rc;
            }
            if (x && (rc = launch_extra(st, c, w0, w1))) return rc;
            if (!staged && c > 0 && (rc = download(c - 1))) return rc;
        }
        if (staged) {
            HIP_TRY(hipMemcpyAsync(ctx.pinned + out_begin, ctx.arena + out_begin, out_end - out_begin, hipMemcpyDeviceToHost, ctx.s[0]));
            HIP_TRY(hipStreamSynchronize(ctx.s[0]));
            for (const OutArray &o : outs)
                if (o.copied_back() && o.slot.bytes) memcpy(o.host, ctx.pinned + (o.dev - ctx.arena), o.slot.bytes);
        } else {
            if ((rc = download(n_chunks - 1))) return rc;
            HIP_TRY(hipStreamSynchronize(ctx.s[0]));
            HIP_TRY(hipStreamSynchronize(ctx.s[1]));
        }
        if (audit_on) HIP_TRY(hipMemcpy(x->audit_report, report_dev, DD_AUDIT_REPORT_BYTES(x->audit_max_records), hipMemcpyDeviceToHost));
        return DD_SUCCESS;
    }
};

int compute_likelihoods_impl(Model model, const dd_params *p, const dd_batch *b, dd_result *r, int device, uint32_t options = 0,
                             const ExtraRequest *x = nullptr)
{
    HostCall call{model, p, b, r, device, options, x};
    return call.run();
}

// One persistent host thread per block slot: its thread_local device cache (arena, pinned mirror, streams) survives between
// calls, which per-call threads would allocate and free every time.  The threads wait for work for the life of the process.
class SlotWorker {
public:
    SlotWorker() : has_job_(false), done_(true) { th_ = std::thread([this]() { loop(); }); th_.detach(); }
    void submit(std::function<void()> f)
    {
        std::unique_lock<std::mutex> lk(m_);
        job_ = std::move(f); has_job_ = true; done_ = false;
        cv_.notify_all();
    }
    void wait()
    {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [this]() { return done_; });
    }
private:
    void loop()
    {
        for (;;) {
            std::function<void()> f;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [this]() { return has_job_; });
                f = std::move(job_); has_job_ = false;
            }
            f();
            {
                std::unique_lock<std::mutex> lk(m_);
                done_ = true;
                cv_.notify_all();
            }
        }
    }
    std::thread th_;
    std::mutex m_;
    std::condition_variable cv_;
    std::function<void()> job_;
    bool has_job_, done_;
};

std::mutex g_multi_mutex;                       // one multi-device call at a time per process (the slots are shared)
std::vector<SlotWorker *> g_slots;              // never destroyed: the threads outlive static destruction

int compute_multi(Model model, const dd_params *p, const dd_batch *b, dd_result *r, const int *devices, int n)
{
    if (!devices || n < 1) return fail(DD_ERR_INVALID, "dd_compute_likelihoods_multi: no devices");
    if (n == 1) return compute_likelihoods_impl(model, p, b, r, devices[0]);
    dd_sizes sz;
    int rc = front_checks(p, b, r, sz);
    if (rc || sz.n_pairs == 0) return rc;
    const int W = b->n_windows;
    std::vector<int32_t> bounds((size_t)n + 1);
    if ((rc = dd_partition_windows(b, n, bounds.data()))) return rc;
    std::vector<int64_t> pair_off((size_t)W + 1), hpos_off((size_t)W + 1), vc_off((size_t)W + 1);
    dd_batch_offsets(b, pair_off.data(), hpos_off.data(), vc_off.data());
    const ResultIndex idx = {pair_off.data(), hpos_off.data(), vc_off.data(), b->win_read_off};

    struct Block {
        std::vector<int32_t> win_hap_off, win_read_off, hap_seq_off, read_seq_off, hap_var_off;
        dd_batch b; dd_result r; int rc; std::string err;
    };
    std::vector<std::unique_ptr<Block> > blocks;
    for (int i = 0; i < n; i++) {
        const int w0 = bounds[(size_t)i], w1 = bounds[(size_t)i + 1];
        std::unique_ptr<Block> B(new Block());
        B->rc = DD_SUCCESS;
        const int h0 = b->win_hap_off[w0], h1 = b->win_hap_off[w1], q0 = b->win_read_off[w0], q1 = b->win_read_off[w1];
        const int hs0 = b->hap_seq_off[h0], rs0 = b->read_seq_off[q0];
        const int v0 = b->hap_var_off ? b->hap_var_off[h0] : 0;
        // offset arrays rebased to the block; data arrays are the caller's, shifted
        for (int w = w0; w <= w1; w++) { B->win_hap_off.push_back(b->win_hap_off[w] - h0); B->win_read_off.push_back(b->win_read_off[w] - q0); }
        for (int h = h0; h <= h1; h++) {
            B->hap_seq_off.push_back(b->hap_seq_off[h] - hs0);
            if (b->hap_var_off) B->hap_var_off.push_back(b->hap_var_off[h] - v0);
        }
        for (int q = q0; q <= q1; q++) B->read_seq_off.push_back(b->read_seq_off[q] - rs0);
        dd_batch &s = B->b;
        s = *b;
        s.n_windows = w1 - w0;
        s.win_hap_off = B->win_hap_off.data(); s.win_read_off = B->win_read_off.data();
        s.win_hap_start = b->win_hap_start ? b->win_hap_start + w0 : nullptr;
        s.hap_seq_off = B->hap_seq_off.data(); s.hap_seq = b->hap_seq ? b->hap_seq + hs0 : nullptr;
        s.hap_var_off = b->hap_var_off ? B->hap_var_off.data() : nullptr;
        s.hap_var = b->hap_var ? b->hap_var + 2 * (size_t)v0 : nullptr;
        s.hap_var_flank = b->hap_var_flank ? b->hap_var_flank + 3 * (size_t)v0 : nullptr;
        s.read_seq_off = B->read_seq_off.data();
        s.read_seq = b->read_seq ? b->read_seq + rs0 : nullptr;
        s.read_qidx = b->read_qidx ? b->read_qidx + rs0 : nullptr;
        s.read_mqidx = b->read_mqidx ? b->read_mqidx + q0 : nullptr;
        s.read_start = b->read_start ? b->read_start + q0 : nullptr;
        s.read_flags = b->read_flags ? b->read_flags + q0 : nullptr;
        s.read_mate_pos = b->read_mate_pos ? b->read_mate_pos + q0 : nullptr;
        s.read_mate_len = b->read_mate_len ? b->read_mate_len + q0 : nullptr;
        s.read_lib = b->read_lib ? b->read_lib + q0 : nullptr;
        dd_result &o = B->r;
        memset(&o, 0, sizeof(o));
#define SHIFT(f, space, in_place) o.f = r->f ? r->f + idx.at(SPACE_##space, w0) : nullptr;
        DD_RESULT_FIELDS(SHIFT)
#undef SHIFT
        blocks.push_back(std::move(B));
    }
    std::lock_guard<std::mutex> g(g_multi_mutex);
    while ((int)g_slots.size() < n) g_slots.push_back(new SlotWorker());
    for (int i = 0; i < n; i++) {
        Block *B = blocks[(size_t)i].get();
        const int dev = devices[i];
        g_slots[(size_t)i]->submit([B, model, p, dev]() {
            B->rc = compute_likelihoods_impl(model, p, &B->b, &B->r, dev);
            if (B->rc != DD_SUCCESS) B->err = g_err;          // the worker thread's message
        });
    }
    for (int i = 0; i < n; i++) g_slots[(size_t)i]->wait();
    for (int i = 0; i < n; i++)
        if (blocks[(size_t)i]->rc != DD_SUCCESS)
            return fail(blocks[(size_t)i]->rc, "block " + std::to_string(i) + " (device " + std::to_string(devices[i]) + "): " + blocks[(size_t)i]->err);
    return DD_SUCCESS;
}
} // namespace
} // namespace ddh
using namespace ddh;
// What dd_map_pairs and dd_pair_sums start with: the batch's sizes, the device, the pair and haplotype-pair offsets, and this thread's arena
// with the three offset arrays, hh_off and ll uploaded; more_bytes(c) is what the caller places behind them.  `nothing`: there is nothing to
// compute (no window; needs_hap_pairs: no haplotype pair) and nothing was reserved.
struct PairSumCall {
    dd_sizes sz;
    int W = 0;
    std::vector<int64_t> pair_off, hh_off;
    size_t ns = 0;                                      // hh_off[W]: the batch's haplotype pairs
    dd_device_batch db = {};
    const int64_t *hh_dev = nullptr;
    const double *ll_dev = nullptr;
    DevBuf dev{g_ctx.c};
    bool nothing = true;
};
template <class MoreBytes>
int pair_sum_prologue(PairSumCall &c, const dd_batch *b, const double *ll_host, bool args_given, int device, const char *no_device,
                      bool needs_hap_pairs, MoreBytes more_bytes)
{
    int rc = dd_batch_sizes(b, &c.sz);
    if (rc) return rc;
    if (!args_given) return fail(DD_ERR_INVALID, "null argument");
    if ((rc = use_device(device, no_device))) return rc;
    const int W = c.W = b->n_windows;
    if (W <= 0) return DD_SUCCESS;
    c.pair_off.resize(W + 1); c.hh_off.resize(W + 1);
    dd_batch_offsets(b, c.pair_off.data(), nullptr, nullptr);
    dd_pair_sum_offsets(b, c.hh_off.data());
    c.ns = (size_t)c.hh_off[W];
    if (needs_hap_pairs && c.ns == 0) return DD_SUCCESS;
    if ((rc = g_ctx.c.reserve(device, (size_t)(W + 1) * (2 * 4 + 2 * 8) + (size_t)c.sz.n_pairs * 8 + 5 * 256 + more_bytes(c), 0))) return rc;
    c.db.n_windows = W;
    if ((rc = c.dev.upload(&c.db.win_hap_off, b->win_hap_off, (size_t)W + 1))) return rc;
    if ((rc = c.dev.upload(&c.db.win_read_off, b->win_read_off, (size_t)W + 1))) return rc;
    if ((rc = c.dev.upload(&c.db.win_pair_off, (const int64_t *)c.pair_off.data(), c.pair_off.size()))) return rc;
    if ((rc = c.dev.upload(&c.hh_dev, (const int64_t *)c.hh_off.data(), c.hh_off.size()))) return rc;
    if ((rc = c.dev.upload(&c.ll_dev, ll_host, (size_t)c.sz.n_pairs))) return rc;
    c.nothing = false;
    return DD_SUCCESS;
}

extern "C" {
int dd_last_direct_outputs(void) { return g_last_direct; }

void dd_release_cache(void)
{   // frees this host thread's cached device arena, pinned mirror and streams
    g_ctx.c.release();
}

int dd_reserve_cache(int device, size_t device_bytes, size_t pinned_bytes)
{
    const int rc = use_device(device, "no HIP device: the likelihood path has no CPU fallback");
    return rc ? rc : g_ctx.c.reserve(device, device_bytes, pinned_bytes);
}

void *dd_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
void dd_host_free(void *p)
{
    if (p) (void)hipHostFree(p);
}
int dd_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int dd_map_pairs(const dd_batch *b, const double *ll_host, const double *prior_host, const uint8_t *filtered_host,
                 const int32_t *ncand_host, double *pair_sum_out, double *posterior_out, int32_t *pairs_out, double *vals_out, int device)
{
    PairSumCall c;
    int rc = pair_sum_prologue(c, b, ll_host, ll_host && prior_host && filtered_host && ncand_host && pairs_out && vals_out, device,
                               "no HIP device: the genotype reduction has no CPU fallback in this library", false,
                               [](const PairSumCall &c) { return 3 * c.ns * 8 + (size_t)c.sz.n_haps * 5 + (size_t)c.W * 40 + 27 * 256; });
    if (rc || c.nothing) return rc;
    DevBuf &dev = c.dev;
    const size_t ns = c.ns, W = (size_t)c.W;
    const double *prior_dev = nullptr;
    const uint8_t *filt_dev = nullptr;
    const int32_t *nc_dev = nullptr;
    double *sum_dev = nullptr, *post_dev = nullptr, *vals_dev = nullptr;
    int32_t *pairs_dev = nullptr;
    if ((rc = dev.upload(&prior_dev, prior_host, ns))) return rc;
    if ((rc = dev.upload(&filt_dev, filtered_host, (size_t)c.sz.n_haps))) return rc;
    if ((rc = dev.upload(&nc_dev, ncand_host, (size_t)c.sz.n_haps))) return rc;
    if ((rc = dev.alloc(&sum_dev, ns))) return rc;
    if ((rc = dev.alloc(&post_dev, ns))) return rc;
    if ((rc = dev.alloc(&vals_dev, 3 * W))) return rc;
    if ((rc = dev.alloc(&pairs_dev, 4 * W))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if ((rc = dd_pair_sums_device(&c.db, c.hh_dev, c.hh_off[W], c.ll_dev, sum_dev, nullptr))) return rc;
    if ((rc = dd_map_pairs_device(&c.db, c.hh_dev, sum_dev, prior_dev, filt_dev, nc_dev, post_dev, pairs_dev, vals_dev, nullptr))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (pair_sum_out) HIP_TRY(hipMemcpy(pair_sum_out, sum_dev, ns * sizeof(double), hipMemcpyDeviceToHost));
    if (posterior_out) HIP_TRY(hipMemcpy(posterior_out, post_dev, ns * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pairs_out, pairs_dev, 4 * W * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(vals_out, vals_dev, 3 * W * sizeof(double), hipMemcpyDeviceToHost));
    return DD_SUCCESS;
}

int dd_pair_sums(const dd_batch *b, const double *ll_host, double *out_host, int device)
{
    PairSumCall c;
    int rc = pair_sum_prologue(c, b, ll_host, ll_host && out_host, device, "no HIP device: the genotype read-sum has no CPU fallback in this library",
                               true, [](const PairSumCall &c) { return c.ns * 8 + 11 * 256; });
    if (rc || c.nothing) return rc;
    double *out_dev = nullptr;
    if ((rc = c.dev.alloc(&out_dev, c.ns))) return rc;
    if ((rc = dd_pair_sums_device(&c.db, c.hh_dev, c.hh_off[(size_t)c.W], c.ll_dev, out_dev, nullptr))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out_host, out_dev, c.ns * sizeof(double), hipMemcpyDeviceToHost));
    return DD_SUCCESS;
}
int dd_compute_likelihoods(const dd_params *p, const dd_batch *b, dd_result *r, int device)
{
    return compute_likelihoods_impl(MODEL_FBMAXERR, p, b, r, device);
}
// the options of the main model's host-pointer entries: long windows, and with them wide deletions
static int check_main_options(uint32_t options)
{
    if (options & ~(DD_OPT_LONG_WINDOWS | DD_OPT_WIDE_DELETIONS)) return fail(DD_ERR_INVALID, "unknown option bits");
    if ((options & DD_OPT_WIDE_DELETIONS) && !(options & DD_OPT_LONG_WINDOWS))
        return fail(DD_ERR_INVALID, "DD_OPT_WIDE_DELETIONS needs DD_OPT_LONG_WINDOWS (the wide build is the long-window kernel's)");
    return DD_SUCCESS;
}
int dd_compute_likelihoods_ex(const dd_params *p, const dd_batch *b, dd_result *r, int device, uint32_t options)
{
    if (check_main_options(options)) return DD_ERR_INVALID;
    return compute_likelihoods_impl(MODEL_FBMAXERR, p, b, r, device, options);
}
int dd_compute_likelihoods_cigars(const dd_params *p, const dd_batch *b, dd_result *r, const int32_t *hap_ref_pos, const uint8_t *hap_aligned,
                                  const dd_cigar_result *cig, int ops_cap, int device, uint32_t options)
{
    if (check_main_options(options)) return DD_ERR_INVALID;
    if (!hap_ref_pos) return fail(DD_ERR_INVALID, "dd_compute_likelihoods_cigars: hap_ref_pos is required (Haplotype::refHpos per haplotype base)");
    if (ops_cap < 1) return fail(DD_ERR_INVALID, "dd_compute_likelihoods_cigars: ops_cap must be at least 1");
    if (!cig || !cig->n_ops || !cig->ops || !cig->ref_off || !cig->status)
        return fail(DD_ERR_INVALID, "dd_compute_likelihoods_cigars: every array of dd_cigar_result is required");
    ExtraRequest x = {hap_ref_pos, hap_aligned, ops_cap, false};
    x.cigars = *cig;
    return compute_likelihoods_impl(MODEL_FBMAXERR, p, b, r, device, options, &x);
}
int dd_compute_likelihoods_realign(const dd_params *p, const dd_batch *b, dd_result *r, int mode, const int32_t *win_hap_pair,
                                   const int32_t *hap_n_indels, const int32_t *hap_ref_pos, const uint8_t *hap_aligned,
                                   const dd_realign_result *out, int ops_cap, int device, uint32_t options)
{
    if (check_main_options(options)) return DD_ERR_INVALID;
    if (mode != DD_REALIGN_FIRST_MAX && mode != DD_REALIGN_PAIR) return fail(DD_ERR_INVALID, "dd_compute_likelihoods_realign: unknown mode");
    if (mode == DD_REALIGN_PAIR && (!win_hap_pair || !hap_n_indels))
        return fail(DD_ERR_INVALID, "dd_compute_likelihoods_realign: DD_REALIGN_PAIR needs win_hap_pair and hap_n_indels");
    if (!hap_ref_pos) return fail(DD_ERR_INVALID, "dd_compute_likelihoods_realign: hap_ref_pos is required (Haplotype::refHpos per haplotype base)");
    if (ops_cap < 1) return fail(DD_ERR_INVALID, "dd_compute_likelihoods_realign: ops_cap must be at least 1");
    if (!out || !out->hap || !out->status || !out->n_ops || !out->ops || !out->ref_off)
        return fail(DD_ERR_INVALID, "dd_compute_likelihoods_realign: every array of dd_realign_result is required");
    ExtraRequest x = {hap_ref_pos, hap_aligned, ops_cap, true};
    x.mode = mode; x.win_hap_pair = win_hap_pair; x.hap_n_indels = hap_n_indels; x.reads = *out;
    return compute_likelihoods_impl(MODEL_FBMAXERR, p, b, r, device, options, &x);
}
int dd_compute_likelihoods_realign_diploid(const dd_params *p, const dd_batch *b, dd_result *r, const double *prior, const int32_t *hap_n_indels,
                                           const int32_t *hap_ref_pos, const uint8_t *hap_aligned, const dd_diploid_pair_result *pair_out,
                                           const dd_realign_result *realign_out, int ops_cap, int device, uint32_t options)
{
    if (check_main_options(options)) return DD_ERR_INVALID;
    if (!prior || !hap_n_indels) return fail(DD_ERR_INVALID, "dd_compute_likelihoods_realign_diploid: prior and hap_n_indels are required");
    if (!hap_ref_pos) return fail(DD_ERR_INVALID, "dd_compute_likelihoods_realign_diploid: hap_ref_pos is required (Haplotype::refHpos per haplotype base)");
    if (ops_cap < 1) return fail(DD_ERR_INVALID, "dd_compute_likelihoods_realign_diploid: ops_cap must be at least 1");
    if (!pair_out || !pair_out->pair || !pair_out->state || !pair_out->best || !pair_out->gap || !pair_out->margin)
        return fail(DD_ERR_INVALID, "dd_compute_likelihoods_realign_diploid: every array of dd_diploid_pair_result is required");
    if (!realign_out || !realign_out->hap || !realign_out->status || !realign_out->n_ops || !realign_out->ops || !realign_out->ref_off)
        return fail(DD_ERR_INVALID, "dd_compute_likelihoods_realign_diploid: every array of dd_realign_result is required");
    ExtraRequest x = {hap_ref_pos, hap_aligned, ops_cap, true};
    x.mode = DD_REALIGN_PAIR; x.hap_n_indels = hap_n_indels; x.reads = *realign_out;
    x.diploid = true; x.prior = prior; x.pairs = *pair_out;
    return compute_likelihoods_impl(MODEL_FBMAXERR, p, b, r, device, options, &x);
}
int dd_compute_likelihoods_faster(const dd_params *p, const dd_batch *b, dd_result *r, int device)
{
    return compute_likelihoods_impl(MODEL_S, p, b, r, device);
}
int dd_compute_likelihoods_faster_ex(const dd_params *p, const dd_batch *b, dd_result *r, int device, uint32_t options)
{
    if (options & ~(DD_OPT_LONG_WINDOWS_FASTER | DD_OPT_WIDE_DELETIONS)) return fail(DD_ERR_INVALID, "unknown option bits");
    return compute_likelihoods_impl(MODEL_S, p, b, r, device, options);
}
int dd_compute_likelihoods_faster_keys(const dd_params *p, const dd_batch *b, dd_result *r, int16_t *keys_out, int device, uint32_t options)
{
    // DD_OPT_WIDE_DELETIONS is taken where it is needed (maxLengthDel above 31); beside a smaller value it stays an unknown bit of this entry
    if (options & ~(DD_OPT_LONG_WINDOWS_FASTER | (wide_on(p, options) ? DD_OPT_WIDE_DELETIONS : 0u))) return fail(DD_ERR_INVALID, "unknown option bits");
    if (!keys_out) return fail(DD_ERR_INVALID, "dd_compute_likelihoods_faster_keys: keys_out is required");
    ExtraRequest x = {};
    x.keys = keys_out;
    return compute_likelihoods_impl(MODEL_S, p, b, r, device, options, &x);
}
int dd_compute_likelihoods_audit(const dd_params *p, const dd_batch *b, dd_result *r, int device, uint32_t options, uint64_t seed, int32_t n_want,
                                 void *report, int64_t max_records)
{
    if (options & ~DD_OPT_LONG_WINDOWS) return fail(DD_ERR_INVALID, "dd_compute_likelihoods_audit: unknown option bits (the --faster model takes no audit)");
    if (!report) return fail(DD_ERR_INVALID, "dd_compute_likelihoods_audit: report is required");
    if (max_records < 0) return fail(DD_ERR_INVALID, "dd_compute_likelihoods_audit: negative max_records");
    memset(report, 0, DD_AUDIT_REPORT_BYTES(max_records));   // a batch without pairs, or nothing chosen: an empty report
    ExtraRequest x = {};
    x.audit = true; x.audit_seed = seed; x.audit_want = n_want; x.audit_report = report; x.audit_max_records = max_records;
    return compute_likelihoods_impl(MODEL_FBMAXERR, p, b, r, device, options, &x);
}
int dd_compute_likelihoods_faster_audit(const dd_params *p, const dd_batch *b, dd_result *r, int16_t *keys_out, int device, uint32_t options,
                                        uint64_t seed, int32_t n_want, void *report, int64_t max_records)
{
    if (options & ~DD_OPT_LONG_WINDOWS_FASTER)
        return fail(DD_ERR_INVALID, "dd_compute_likelihoods_faster_audit: unknown option bits (0 or DD_OPT_LONG_WINDOWS_FASTER)");
    if (!report) return fail(DD_ERR_INVALID, "dd_compute_likelihoods_faster_audit: report is required");
    if (max_records < 0) return fail(DD_ERR_INVALID, "dd_compute_likelihoods_faster_audit: negative max_records");
    memset(report, 0, DD_AUDIT_REPORT_BYTES(max_records));                // a batch without pairs, or an empty sample: an empty report
    ExtraRequest x = {};
    x.keys = keys_out;
    x.audit = true; x.audit_seed = seed; x.audit_want = n_want; x.audit_report = report; x.audit_max_records = max_records;
    return compute_likelihoods_impl(MODEL_S, p, b, r, device, options, &x);
}

// test hook, see include/dindel_hmm.h
void dd_audit_inject_next(int window) { g_audit_inject = window; }
int dd_compute_likelihoods_multi(const dd_params *p, const dd_batch *b, dd_result *r, const int *devices, int n_devices)
{
    return compute_multi(MODEL_FBMAXERR, p, b, r, devices, n_devices);
}
int dd_compute_likelihoods_faster_multi(const dd_params *p, const dd_batch *b, dd_result *r, const int *devices, int n_devices)
{
    return compute_multi(MODEL_S, p, b, r, devices, n_devices);
}
} // extern "C"
