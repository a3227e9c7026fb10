// host_path.cpp — the host-pointer entry points of the C ABI: the per-thread device arena and stream cache, validation, staging,
// chunked double-buffered execution, and the front end for several devices of one process.
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include "capi_internal.h"

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
    template <class T> int alloc(T **out, size_t n)
    {
        const size_t off = align(used), bytes = (n ? n : 1) * sizeof(T);
        if (off + bytes > C.arena_cap) return fail(DD_ERR_HIP, "internal: device arena under-sized");
        used = off + bytes;
        *out = reinterpret_cast<T *>(C.arena + off);
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

// makes `device` current; no_device: the text when the machine has none
int use_device(int device, const char *no_device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(DD_ERR_NO_DEVICE, no_device);
    if (device < 0 || device >= ndev) return fail(DD_ERR_NO_DEVICE, "device ordinal out of range");
    HIP_TRY(hipSetDevice(device));
    return DD_SUCCESS;
}

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
    int64_t at(ResultSpace s, int w) const { return s == SPACE_PAIR ? pair_off[w] : s == SPACE_HPOS ? hpos_off[w] : s == SPACE_VARCOV ? varcov_off[w] : read_off[w]; }
};

// What a host-pointer call checks first; sz: the batch's sizes.  A batch without pairs (sz.n_pairs == 0) is finished here.
int front_checks(const dd_params *p, const dd_batch *b, dd_result *r, dd_sizes &sz)
{
    int rc = check_params(p);
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

// dd_compute_likelihoods_cigars: the haplotypes' reference positions in, the pairs' CIGARs out (host pointers)
// dd_compute_likelihoods_realign: the same inputs, the window pairs and indel counts of its PAIR mode, and per READ the chosen haplotype with
// its CIGAR out (rl != nullptr: the per-pair arrays of `out` are then neither allocated nor filled)
struct RealignRequest {
    int mode; const int32_t *win_hap_pair, *hap_n_indels;
    dd_realign_result out;
};
struct CigarRequest {
    const int32_t *hap_ref_pos; const uint8_t *hap_aligned;
    dd_cigar_result out; int ops_cap;
    const RealignRequest *rl;
};

int compute_likelihoods_impl(Model model, const dd_params *p, const dd_batch *b, dd_result *r, int device, uint32_t options = 0,
                             const CigarRequest *cg = nullptr)
{
    StageClock clk;
    launch_log_clear();
    g_long.log.clear();
    g_flong.log.clear();
    dd_sizes sz;
    int rc = front_checks(p, b, r, sz);
    if (!rc && sz.n_pairs == 0 && cg && cg->rl)              // reads without haplotypes: no pair, nothing to launch, every read marked
        for (int64_t q = 0; q < sz.n_reads; q++) {
            const dd_realign_result &o = cg->rl->out;
            o.hap[q] = -1; o.status[q] = DD_REALIGN_NO_HAPS; o.n_ops[q] = 0; o.ref_off[q] = -1;
        }
    if (rc || sz.n_pairs == 0) return rc;
    // validate content
    if (!b->hap_seq || !b->read_seq || !b->read_qidx || !b->read_mqidx || !b->read_start || !b->read_flags ||
        !b->win_hap_start || !b->qual_table || !b->mapq_table)
        return fail(DD_ERR_INVALID, "null input array");
    if (b->n_qual < 1 || b->n_qual > DD_MAX_QUAL_TABLE || b->n_mapq < 1 || b->n_mapq > DD_MAX_QUAL_TABLE)
        return fail(DD_ERR_INVALID, "quality tables must hold 1..256 entries");
    // windows whose shape the kernels do not cover are skipped one by one (DD_PAIR_UNSUPPORTED), not the batch
    std::vector<uint8_t> win_skip((size_t)b->n_windows);
    int32_t ok_max[2] = {0, 0};
    if (!b->hap_seq_off || !b->read_seq_off) return fail(DD_ERR_INVALID, "null offset array");
    uint8_t sym_lut[256];
    const int sym_left = assign_symbols(b, sym_lut);     // > 0: more than 26 distinct non-ACGTN haplotype bytes in the batch
    if (sym_left < 0) return sym_left;
    clk.mark("symbols");
    // long windows (DD_OPT_LONG_WINDOWS): win_skip holds the classes; the main kernels skip both non-zero classes, the long launch that
    // follows each block's main launches computes class 2
    // (DD_OPT_LONG_WINDOWS_FASTER: the same for the --faster model, with its own classes and its own kernel)
    const bool fl_on = model == MODEL_S && (options & DD_OPT_LONG_WINDOWS_FASTER);
    const bool long_on = (model == MODEL_FBMAXERR && (options & DD_OPT_LONG_WINDOWS)) || fl_on;
    LongPath &long_path = fl_on ? g_flong : g_long;           // the model's long path (used only if long_on)
    int32_t long_max[4] = {0, 0, 0, 0};
    int n_skip;
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
    std::vector<double> lib_logprob, lib_log95;
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
    if ((rc = use_device(device, "no HIP device: the likelihood path has no CPU fallback"))) return rc;

    const int W = b->n_windows;
    std::vector<int32_t> hap_window((size_t)sz.n_haps);
    std::vector<int64_t> pair_off(W + 1), hpos_off(W + 1), vc_off(W + 1);
    dd_build_index(b, hap_window.data(), pair_off.data(), hpos_off.data(), vc_off.data());
    std::vector<double> tables(DD_TABLE_DOUBLES);
    rc = dd_build_tables(p, b->qual_table, b->n_qual, b->mapq_table, b->n_mapq, tables.data());
    if (rc < 0) return rc;

    // ---- host-side planning first (no device work yet): launch classes and scratch size ----
    // Ragged batches: one launch per (lane tiling of the haplotypes, read-length interval) that has work (build_launch_classes) — a single
    // 170-bp haplotype or 250-bp read does not drag every pair of the batch onto the K = 3 / long-read build.
    dd_length_classes lcls;
    std::vector<int32_t> class_list;
    memset(&lcls, 0, sizeof(lcls));
    if (model == MODEL_FBMAXERR && !getenv("DD_NO_LENGTH_CLASSES")) {                      // env: A/B only
        class_list.resize((size_t)sz.n_haps * DD_N_READ_CLASSES + 1);
        if ((rc = build_launch_classes(b, n_skip ? win_skip.data() : nullptr, p, class_list.data(), &lcls))) return rc;
    }
    const int32_t *class_list_dev = nullptr;
    dd_device_batch db;
    memset(&db, 0, sizeof(db));
    db.n_windows = W; db.n_haps = (int32_t)sz.n_haps; db.n_reads = (int32_t)sz.n_reads;
    db.max_hap_len = sz.max_hap_len; db.max_read_len = sz.max_read_len;
    db.n_qual = b->n_qual; db.n_mapq = b->n_mapq;
    for (int w = 0; w < W; w++)
        if (!win_skip[(size_t)w] && b->win_read_off[w + 1] - b->win_read_off[w] > db.max_window_reads) db.max_window_reads = b->win_read_off[w + 1] - b->win_read_off[w];
    size_t ws_bytes = model == MODEL_S ? 0 : dd_workspace_bytes(p, &db);
    const bool single_class = lcls.n_launches <= 1;
    if (!single_class) {
        db.classes = &lcls;
        db.hap_class_list = class_list.data();             // (host pointer: only dd_workspace_bytes' class walk looks at it here)
        const size_t w2 = dd_workspace_bytes(p, &db);
        if (w2 > ws_bytes) ws_bytes = w2;
        db.classes = nullptr; db.hap_class_list = nullptr;
    }

    size_t lws_bytes = 0;                                   // long path: its own workspace per stream
    if (long_on && long_max[2] > 0) {
        db.long_max_hap_len = long_max[2]; db.long_max_read_len = long_max[3];
        lws_bytes = long_path.workspace_bytes(p, &db);
        if (!lws_bytes) return fail(DD_ERR_UNSUPPORTED, "long path: no plan for this shape");
    }

    clk.mark("plan");
    // ---- device arena (cached per host thread) ----
    const size_t np = (size_t)sz.n_pairs;
    const size_t n_var = b->hap_var_off ? (size_t)b->hap_var_off[sz.n_haps] : 0;
    const size_t in_bytes = (size_t)(W + 1) * (4 + 4 + 8 + 8 + 8) + (size_t)W * 4 + (size_t)(sz.n_haps + 1) * 8 + (size_t)sz.hap_bases +
                            (size_t)(sz.n_reads + 1) * 4 + (size_t)sz.read_bases * 2 + (size_t)sz.n_reads * 6 + n_var * 20 +
                            (size_t)sz.n_haps * 4 + (size_t)lcls.list_len * 4 + 64 + DD_TABLE_DOUBLES * 8 + 48 * 256 + (size_t)W + 256 +
                            (lib_log95.empty() ? 0 : (size_t)sz.n_reads * 9 + (lib_logprob.size() + lib_log95.size()) * 8 + (size_t)(b->n_libs + 1) * 4);
    const RealignRequest *rl = cg ? cg->rl : nullptr;
    const size_t nr = (size_t)sz.n_reads;
    const size_t cigar_in = cg ? (size_t)sz.hap_bases * 4 + (size_t)sz.n_haps + 2 * 256 + (rl ? (size_t)W * 8 + (size_t)sz.n_haps * 4 + 2 * 256 : 0) : 0;
    const size_t cigar_out = !cg ? 0 : rl ? nr * (16 + 4 * (size_t)cg->ops_cap) + 5 * 256 : np * (12 + 4 * (size_t)cg->ops_cap) + 4 * 256;
    const size_t out_bytes = np * (4 * 8 + 2 + 8 * 2 + 4) + (size_t)sz.hpos_len * 2 + 2 * (size_t)sz.var_cov_len + (size_t)sz.n_reads + 24 * 256 + cigar_out;
    const bool staged = in_bytes + cigar_in + out_bytes <= (size_t)64 << 20;    // small batch: one H2D, one D2H through the pinned mirror
    DeviceCtx &ctx = g_ctx.c;
    const size_t long_bytes = lws_bytes ? 2 * (lws_bytes + 256) + 32 * 64 + 256 : 0;
    if ((rc = ctx.reserve(device, in_bytes + cigar_in + out_bytes + 2 * (ws_bytes + 256) + long_bytes, staged ? in_bytes + cigar_in + out_bytes : 0))) return rc;
    clk.mark("reserve");
    DevBuf dev(ctx);
    dev.staged = staged;
#define UP(field, n) if ((rc = dev.upload(&db.field, b->field, (size_t)(n)))) return rc
    UP(win_hap_off, W + 1); UP(win_read_off, W + 1); UP(win_hap_start, W);
    UP(hap_seq_off, sz.n_haps + 1); UP(hap_seq, sz.hap_bases);
    UP(read_seq_off, sz.n_reads + 1);
    // The two big inputs (one byte per read base each).  Large batches: only reserved here — each window block's share is copied
    // on the block's own stream right in front of its kernels, so all but the first block's transfer hides behind the kernels of
    // the block before.
    const bool late_reads = !staged && sz.read_bases > 0;
    char *d_read_seq = nullptr; uint8_t *d_read_qidx = nullptr;
    if (late_reads) {
        if ((rc = dev.alloc(&d_read_seq, (size_t)sz.read_bases))) return rc;
        if ((rc = dev.alloc(&d_read_qidx, (size_t)sz.read_bases))) return rc;
        db.read_seq = d_read_seq; db.read_qidx = d_read_qidx;
    } else {
        // Staged (small) batches whose two big inputs the caller keeps in page-locked, device-addressable memory (the C++ adapter packs
        // into dd_host_alloc buffers): the kernels read them in place over the link — each (read, haplotype) pair fetches its read once,
        // ~80 MB per 256-window batch at 8 haplotypes — instead of waiting for a staged copy whose blit kernels share the CUs with the
        // batch that is running (profiles/r03/window_loop_timeline.txt).  DD_ZERO_COPY_IN=0 switches it off (A/B).
        static const bool zero_copy_in = !(getenv("DD_ZERO_COPY_IN") && !strcmp(getenv("DD_ZERO_COPY_IN"), "0"));
        const void *ms = zero_copy_in ? mapped_device_ptr(b->read_seq, (size_t)sz.read_bases) : nullptr;
        const void *mq = zero_copy_in ? mapped_device_ptr(b->read_qidx, (size_t)sz.read_bases) : nullptr;
        if (ms && mq) { db.read_seq = static_cast<const char *>(ms); db.read_qidx = static_cast<const uint8_t *>(mq); }
        else { UP(read_seq, sz.read_bases); UP(read_qidx, sz.read_bases); }
    }
    UP(read_mqidx, sz.n_reads); UP(read_start, sz.n_reads); UP(read_flags, sz.n_reads);
#undef UP
    if (b->hap_var_off) {
        if ((rc = dev.upload(&db.hap_var_off, b->hap_var_off, (size_t)sz.n_haps + 1))) return rc;
        if ((rc = dev.upload(&db.hap_var, b->hap_var, 2 * n_var))) return rc;
        if (b->hap_var_flank && (rc = dev.upload(&db.hap_var_flank, b->hap_var_flank, 3 * n_var))) return rc;
    }
    if ((rc = dev.upload(&db.hap_window, (const int32_t *)hap_window.data(), hap_window.size()))) return rc;
    if ((rc = dev.upload(&db.win_pair_off, (const int64_t *)pair_off.data(), pair_off.size()))) return rc;
    if ((rc = dev.upload(&db.win_hpos_off, (const int64_t *)hpos_off.data(), hpos_off.size()))) return rc;
    if ((rc = dev.upload(&db.win_varcov_off, (const int64_t *)vc_off.data(), vc_off.size()))) return rc;
    if ((rc = dev.upload(&db.tables, (const double *)tables.data(), tables.size()))) return rc;
    if ((rc = dev.upload(&db.sym_lut, (const uint8_t *)sym_lut, (size_t)256))) return rc;
    if (n_skip > 0 && (rc = dev.upload(&db.win_skip, (const uint8_t *)win_skip.data(), win_skip.size()))) return rc;
    if (!lib_log95.empty()) {
        if ((rc = dev.upload(&db.read_mate_pos, b->read_mate_pos, (size_t)sz.n_reads))) return rc;
        if ((rc = dev.upload(&db.read_mate_len, b->read_mate_len, (size_t)sz.n_reads))) return rc;
        if ((rc = dev.upload(&db.read_lib, b->read_lib, (size_t)sz.n_reads))) return rc;
        if ((rc = dev.upload(&db.lib_off, b->lib_off, (size_t)b->n_libs + 1))) return rc;
        if ((rc = dev.upload(&db.lib_logprob, (const double *)lib_logprob.data(), lib_logprob.size()))) return rc;
        if ((rc = dev.upload(&db.lib_log95, (const double *)lib_log95.data(), lib_log95.size()))) return rc;
    }
    if (!single_class && (rc = dev.upload(&class_list_dev, (const int32_t *)class_list.data(), (size_t)lcls.list_len))) return rc;
    const int32_t *hap_ref_pos_dev = nullptr;
    const uint8_t *hap_aligned_dev = nullptr;
    if (cg) {
        if ((rc = dev.upload(&hap_ref_pos_dev, cg->hap_ref_pos, (size_t)sz.hap_bases))) return rc;
        if (cg->hap_aligned && (rc = dev.upload(&hap_aligned_dev, cg->hap_aligned, (size_t)sz.n_haps))) return rc;
    }
    const int32_t *win_hap_pair_dev = nullptr, *hap_n_indels_dev = nullptr;
    if (rl && rl->mode == DD_REALIGN_PAIR) {
        if ((rc = dev.upload(&win_hap_pair_dev, rl->win_hap_pair, (size_t)W * 2))) return rc;
        if ((rc = dev.upload(&hap_n_indels_dev, rl->hap_n_indels, (size_t)sz.n_haps))) return rc;
    }
    if ((rc = dev.flush_uploads(ctx.s[0]))) return rc;       // staged mode: the one H2D copy
    if (!staged) HIP_TRY(hipStreamSynchronize(nullptr));     // pageable uploads went through the null stream's DMA
    clk.mark("upload");

    dd_result dr;
    memset(&dr, 0, sizeof(dr));
    const size_t out_begin = DevBuf::align(dev.used);
    // Output arrays the caller keeps in page-locked host memory that this device can address (dd_host_alloc, hipHostMalloc) are
    // written by the kernels themselves, over the link, as the pairs finish: no staging copy in HBM and no copy afterwards.
    // (The runtime carries device -> host copies of this size out with a copy KERNEL: profiles/r02/hostapi_timeline.txt shows
    // 300 ms of such kernels on the CUs beside 410 ms of HMM kernels for configs[1].)  status and offHapHMQ stay in HBM: the
    // onHap kernel reads them back.  DD_ZERO_COPY=0 switches this off (A/B).
    static const bool zero_copy_on = !(getenv("DD_ZERO_COPY") && !strcmp(getenv("DD_ZERO_COPY"), "0"));
    const ResultIndex idx = {pair_off.data(), hpos_off.data(), vc_off.data(), b->win_read_off};
#define FLAG(f, space, in_place) bool f = false;
    struct { DD_RESULT_FIELDS(FLAG) } direct;
#undef FLAG
    int n_direct = 0;
#define OUT(f, space, in_place) if (r->f) { \
        const size_t n = (size_t)idx.at(SPACE_##space, W); \
        void *m = (in_place && zero_copy_on) ? mapped_device_ptr(r->f, n * sizeof(*r->f)) : nullptr; \
        if (m) { dr.f = static_cast<decltype(dr.f)>(m); direct.f = true; n_direct++; } \
        else if ((rc = dev.alloc(&dr.f, n))) return rc; }
    DD_RESULT_FIELDS(OUT)
#undef OUT
    // a CIGAR request reads hpos on the device: alignments the caller wants in page-locked memory are then staged in HBM and copied back
    // like pageable ones, instead of being read back over the link by the CIGAR kernel
    if (cg && direct.hpos) {
        if ((rc = dev.alloc(&dr.hpos, (size_t)sz.hpos_len))) return rc;
        direct.hpos = false; n_direct--;
    }
    // a realign request reads ll and onHap on the device as well
    if (rl && direct.ll) {
        if ((rc = dev.alloc(&dr.ll, np))) return rc;
        direct.ll = false; n_direct--;
    }
    if (rl && direct.onHap) {
        if ((rc = dev.alloc(&dr.onHap, nr))) return rc;
        direct.onHap = false; n_direct--;
    }
    g_last_direct = n_direct;
    if (r->onHap && !r->offHapHMQ && (rc = dev.alloc(&dr.offHapHMQ, np))) return rc;   // onHap is derived from it
    // CIGARs: the per-base alignments are needed on the device even when the caller does not want them back (r->hpos == NULL: nothing of
    // them is copied), and the CIGAR arrays come back with the other outputs
    dd_cigar_result dcg;
    memset(&dcg, 0, sizeof(dcg));
    dd_realign_result drl;
    memset(&drl, 0, sizeof(drl));
    if (rl) {
        if ((rc = dev.alloc(&drl.hap, nr)) || (rc = dev.alloc(&drl.status, nr)) || (rc = dev.alloc(&drl.n_ops, nr)) ||
            (rc = dev.alloc(&drl.ref_off, nr)) || (rc = dev.alloc(&drl.ops, nr * (size_t)cg->ops_cap))) return rc;
    } else if (cg) {
        if ((rc = dev.alloc(&dcg.n_ops, np)) || (rc = dev.alloc(&dcg.ref_off, np)) || (rc = dev.alloc(&dcg.status, np)) ||
            (rc = dev.alloc(&dcg.ops, np * (size_t)cg->ops_cap))) return rc;
    }
    const size_t out_end = dev.used;
    if (cg && !dr.hpos && (rc = dev.alloc(&dr.hpos, (size_t)sz.hpos_len))) return rc;   // (behind the outputs: not part of the staged copy back)
    unsigned char *ws[2] = {nullptr, nullptr};
    for (int i = 0; i < 2; i++)
        if (ws_bytes && (rc = dev.alloc(&ws[i], ws_bytes))) return rc;
    struct { hipStream_t s[2]; } streams = {{ctx.s[0], ctx.s[1]}};
    unsigned char *lws[2] = {nullptr, nullptr};
    unsigned long long *long_stats = nullptr;               // long_path.n_stats (2 or 4) words per window block's long launch
    if (lws_bytes) {
        for (int i = 0; i < 2; i++)
            if ((rc = dev.alloc(&lws[i], lws_bytes))) return rc;
        if ((rc = dev.alloc(&long_stats, (size_t)4 * 64))) return rc;      // 64 blocks at most, 4 words at most
    }

    // Chunked, double-buffered execution: contiguous window blocks alternate between two streams, and the D2H
    // of block c is issued after the kernel of block c+1 has been enqueued, so the copy engine drains results
    // while the CUs work on the next block (with pageable user memory the copy call blocks the host thread, not
    // the GPU).  Each stream has its own back-pointer scratch.  Small (staged) batches run as one block on stream 0
    // and come back with one D2H through the pinned mirror.
    int n_chunks = staged ? 1 : (int)((sz.n_pairs + 999999) / 1000000);
    if (n_chunks > 64) n_chunks = 64;
    if (n_chunks > W) n_chunks = W;
    if (n_chunks < 1) n_chunks = 1;
    std::vector<int> cw(n_chunks + 1, 0);      // window boundaries with ~equal pair counts
    for (int c = 1; c < n_chunks; c++) {
        const int64_t target = sz.n_pairs * c / n_chunks;
        int w = cw[c - 1];
        while (w < W && pair_off[w] < target) w++;
        cw[c] = w;
    }
    cw[n_chunks] = W;
#define DOWN(f, space, in_place) { \
        const int64_t off = idx.at(SPACE_##space, w0), n = idx.at(SPACE_##space, w1) - off; \
        if (r->f && n && !direct.f) HIP_TRY(hipMemcpyAsync(r->f + off, dr.f + off, (size_t)n * sizeof(*r->f), hipMemcpyDeviceToHost, st)); }
    auto download = [&](int c) -> int {
        hipStream_t st = streams.s[c & 1];
        const int w0 = cw[c], w1 = cw[c + 1];
        DD_RESULT_FIELDS(DOWN)
        if (rl && b->win_read_off[w1] > b->win_read_off[w0]) {
            const size_t q0 = (size_t)b->win_read_off[w0], n = (size_t)b->win_read_off[w1] - q0, cap = (size_t)cg->ops_cap;
            HIP_TRY(hipMemcpyAsync(rl->out.hap + q0, drl.hap + q0, n * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(rl->out.status + q0, drl.status + q0, n * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(rl->out.n_ops + q0, drl.n_ops + q0, n * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(rl->out.ref_off + q0, drl.ref_off + q0, n * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(rl->out.ops + q0 * cap, drl.ops + q0 * cap, n * cap * 4, hipMemcpyDeviceToHost, st));
        } else if (cg && !rl && pair_off[w1] > pair_off[w0]) {
            const size_t p0 = (size_t)pair_off[w0], n = (size_t)(pair_off[w1] - pair_off[w0]), cap = (size_t)cg->ops_cap;
            HIP_TRY(hipMemcpyAsync(cg->out.n_ops + p0, dcg.n_ops + p0, n * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(cg->out.ref_off + p0, dcg.ref_off + p0, n * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(cg->out.status + p0, dcg.status + p0, n * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(cg->out.ops + p0 * cap, dcg.ops + p0 * cap, n * cap * 4, hipMemcpyDeviceToHost, st));
        }
        return DD_SUCCESS;
    };
    auto enqueue_and_collect = [&]() -> int {
    for (int c = 0; c < n_chunks; c++) {
        const int w0 = cw[c], w1 = cw[c + 1];
        const int g0 = b->win_hap_off[w0], g1 = b->win_hap_off[w1], q0 = b->win_read_off[w0], q1 = b->win_read_off[w1];
        if (late_reads && q1 > q0) {
            const size_t s0 = (size_t)b->read_seq_off[q0], sn = (size_t)b->read_seq_off[q1] - s0;
            HIP_TRY(hipMemcpyAsync(d_read_seq + s0, b->read_seq + s0, sn, hipMemcpyHostToDevice, streams.s[c & 1]));
            HIP_TRY(hipMemcpyAsync(d_read_qidx + s0, b->read_qidx + s0, sn, hipMemcpyHostToDevice, streams.s[c & 1]));
        }
        if (single_class) {
            rc = launch_range(model, p, &db, &dr, ws[c & 1], ws_bytes, streams.s[c & 1], g0, g1, q0, q1, n_chunks > 1);
            if (rc) return rc;
        } else {
            // every launch class of this window block, then onHap once
            for (int i = 0; i < lcls.n_launches; i++) {
                const dd_launch_class &L = lcls.launch[i];
                const int32_t *hl = class_list.data() + L.list_off;
                LenClass lc = len_class_of(L, class_list_dev, i == lcls.n_launches - 1);
                lc.list_begin = (int)(std::lower_bound(hl, hl + L.list_len, g0) - hl);
                lc.list_end = (int)(std::lower_bound(hl, hl + L.list_len, g1) - hl);
                rc = launch_range(model, p, &db, &dr, ws[c & 1], ws_bytes, streams.s[c & 1], g0, g1, q0, q1, n_chunks > 1, &lc);
                if (rc) return rc;
            }
        }
        if (lws_bytes) {
            bool any = false;
            for (int w = w0; w < w1 && !any; w++) any = win_skip[(size_t)w] == DD_WIN_LONG;
            if (any && (rc = long_path.launch_range(p, &db, &dr, lws[c & 1], lws_bytes, streams.s[c & 1], w0, w1, q0, q1, long_stats + long_path.n_stats * c))) return rc;
        }
        // the block's CIGARs, behind its likelihood launches on the same stream (its ops start out zero: a pair's unused slots are defined)
        // or the block's realigned reads (reads of windows without haplotypes are marked too: the launch goes by reads, not by pairs)
        if (rl && q1 > q0) {
            HIP_TRY(hipMemsetAsync(drl.ops + (size_t)q0 * cg->ops_cap, 0, (size_t)(q1 - q0) * cg->ops_cap * 4, streams.s[c & 1]));
            const RealignInputs in = {rl->mode, dr.ll, dr.onHap, win_hap_pair_dev, hap_n_indels_dev, dr.hpos, dr.status, hap_ref_pos_dev, hap_aligned_dev};
            if ((rc = launch_realign_range(&db, in, &drl, cg->ops_cap, streams.s[c & 1], q0, q1))) return rc;
        } else if (cg && !rl && pair_off[w1] > pair_off[w0]) {
            HIP_TRY(hipMemsetAsync(dcg.ops + (size_t)pair_off[w0] * cg->ops_cap, 0, (size_t)(pair_off[w1] - pair_off[w0]) * cg->ops_cap * 4, streams.s[c & 1]));
            if ((rc = launch_cigars_range(&db, dr.hpos, dr.status, hap_ref_pos_dev, hap_aligned_dev, &dcg, cg->ops_cap, streams.s[c & 1],
                                          pair_off[w0], pair_off[w1]))) return rc;
        }
        if (!staged && c > 0 && (rc = download(c - 1))) return rc;
    }
    if (staged) {
        HIP_TRY(hipMemcpyAsync(ctx.pinned + out_begin, ctx.arena + out_begin, out_end - out_begin, hipMemcpyDeviceToHost, streams.s[0]));
        HIP_TRY(hipStreamSynchronize(streams.s[0]));
#define BACK(f, space, in_place) { \
            const size_t n = (size_t)idx.at(SPACE_##space, W); \
            if (r->f && n && !direct.f) memcpy(r->f, ctx.pinned + (reinterpret_cast<unsigned char *>(dr.f) - ctx.arena), n * sizeof(*r->f)); }
        DD_RESULT_FIELDS(BACK)
#undef BACK
        if (rl) {
            const size_t cap = (size_t)cg->ops_cap;
            memcpy(rl->out.hap, ctx.pinned + (reinterpret_cast<unsigned char *>(drl.hap) - ctx.arena), nr * 4);
            memcpy(rl->out.status, ctx.pinned + (reinterpret_cast<unsigned char *>(drl.status) - ctx.arena), nr * 4);
            memcpy(rl->out.n_ops, ctx.pinned + (reinterpret_cast<unsigned char *>(drl.n_ops) - ctx.arena), nr * 4);
            memcpy(rl->out.ref_off, ctx.pinned + (reinterpret_cast<unsigned char *>(drl.ref_off) - ctx.arena), nr * 4);
            memcpy(rl->out.ops, ctx.pinned + (reinterpret_cast<unsigned char *>(drl.ops) - ctx.arena), nr * cap * 4);
        } else if (cg) {
            const size_t cap = (size_t)cg->ops_cap;
            memcpy(cg->out.n_ops, ctx.pinned + (reinterpret_cast<unsigned char *>(dcg.n_ops) - ctx.arena), np * 4);
            memcpy(cg->out.ref_off, ctx.pinned + (reinterpret_cast<unsigned char *>(dcg.ref_off) - ctx.arena), np * 4);
            memcpy(cg->out.status, ctx.pinned + (reinterpret_cast<unsigned char *>(dcg.status) - ctx.arena), np * 4);
            memcpy(cg->out.ops, ctx.pinned + (reinterpret_cast<unsigned char *>(dcg.ops) - ctx.arena), np * cap * 4);
        }
    } else {
        if ((rc = download(n_chunks - 1))) return rc;
        HIP_TRY(hipStreamSynchronize(streams.s[0]));
        HIP_TRY(hipStreamSynchronize(streams.s[1]));
    }
    return DD_SUCCESS;
    };
#undef DOWN
    clk.mark("outputs");
    rc = enqueue_and_collect();
    clk.mark("run");
    if (rc != DD_SUCCESS) {
        // kernels / copies already enqueued keep writing into the caller's buffers and this thread's arena: drain both
        // streams before the error is reported, so that neither is reused while still in flight
        const std::string msg = g_err;
        (void)hipStreamSynchronize(streams.s[0]);
        (void)hipStreamSynchronize(streams.s[1]);
        g_err = msg;
    }
    return rc;
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
    dd_sizes sz;
    int rc = dd_batch_sizes(b, &sz);
    if (rc) return rc;
    if (!ll_host || !prior_host || !filtered_host || !ncand_host || !pairs_out || !vals_out) return fail(DD_ERR_INVALID, "null argument");
    if ((rc = use_device(device, "no HIP device: the genotype reduction has no CPU fallback in this library"))) return rc;
    const int W = b->n_windows;
    if (W <= 0) return DD_SUCCESS;
    std::vector<int64_t> pair_off(W + 1), hh_off(W + 1);
    dd_batch_offsets(b, pair_off.data(), nullptr, nullptr);
    dd_pair_sum_offsets(b, hh_off.data());
    const size_t ns = (size_t)hh_off[W];
    DeviceCtx &ctx = g_ctx.c;
    if ((rc = ctx.reserve(device, (size_t)(2 * (W + 1) * 4 + 2 * (W + 1) * 8 + ((size_t)sz.n_pairs + 3 * ns) * 8 + (size_t)sz.n_haps * 5 + (size_t)W * 40 + 32 * 256), 0))) return rc;
    DevBuf dev(ctx);
    dd_device_batch db;
    memset(&db, 0, sizeof(db));
    db.n_windows = W;
    if ((rc = dev.upload(&db.win_hap_off, b->win_hap_off, (size_t)W + 1))) return rc;
    if ((rc = dev.upload(&db.win_read_off, b->win_read_off, (size_t)W + 1))) return rc;
    if ((rc = dev.upload(&db.win_pair_off, (const int64_t *)pair_off.data(), pair_off.size()))) return rc;
    const int64_t *hh_dev = nullptr;
    const double *ll_dev = nullptr, *prior_dev = nullptr;
    const uint8_t *filt_dev = nullptr;
    const int32_t *nc_dev = nullptr;
    double *sum_dev = nullptr, *post_dev = nullptr, *vals_dev = nullptr;
    int32_t *pairs_dev = nullptr;
    if ((rc = dev.upload(&hh_dev, (const int64_t *)hh_off.data(), hh_off.size()))) return rc;
    if ((rc = dev.upload(&ll_dev, ll_host, (size_t)sz.n_pairs))) return rc;
    if ((rc = dev.upload(&prior_dev, prior_host, ns))) return rc;
    if ((rc = dev.upload(&filt_dev, filtered_host, (size_t)sz.n_haps))) return rc;
    if ((rc = dev.upload(&nc_dev, ncand_host, (size_t)sz.n_haps))) return rc;
    if ((rc = dev.alloc(&sum_dev, ns))) return rc;
    if ((rc = dev.alloc(&post_dev, ns))) return rc;
    if ((rc = dev.alloc(&vals_dev, (size_t)3 * W))) return rc;
    if ((rc = dev.alloc(&pairs_dev, (size_t)4 * W))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if ((rc = dd_pair_sums_device(&db, hh_dev, hh_off[W], ll_dev, sum_dev, nullptr))) return rc;
    if ((rc = dd_map_pairs_device(&db, hh_dev, sum_dev, prior_dev, filt_dev, nc_dev, post_dev, pairs_dev, vals_dev, nullptr))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (pair_sum_out) HIP_TRY(hipMemcpy(pair_sum_out, sum_dev, ns * sizeof(double), hipMemcpyDeviceToHost));
    if (posterior_out) HIP_TRY(hipMemcpy(posterior_out, post_dev, ns * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pairs_out, pairs_dev, (size_t)4 * W * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(vals_out, vals_dev, (size_t)3 * W * sizeof(double), hipMemcpyDeviceToHost));
    return DD_SUCCESS;
}

int dd_pair_sums(const dd_batch *b, const double *ll_host, double *out_host, int device)
{
    dd_sizes sz;
    int rc = dd_batch_sizes(b, &sz);
    if (rc) return rc;
    if (!ll_host || !out_host) return fail(DD_ERR_INVALID, "null argument");
    if ((rc = use_device(device, "no HIP device: the genotype read-sum has no CPU fallback in this library"))) return rc;
    const int W = b->n_windows;
    std::vector<int64_t> pair_off(W + 1), hh_off(W + 1);
    dd_batch_offsets(b, pair_off.data(), nullptr, nullptr);
    dd_pair_sum_offsets(b, hh_off.data());
    if (hh_off[W] == 0) return DD_SUCCESS;
    DeviceCtx &ctx = g_ctx.c;
    if ((rc = ctx.reserve(device, (size_t)(2 * (W + 1) * 4 + 2 * (W + 1) * 8 + (sz.n_pairs + hh_off[W]) * 8 + 16 * 256), 0))) return rc;
    DevBuf dev(ctx);
    dd_device_batch db;
    memset(&db, 0, sizeof(db));
    db.n_windows = W;
    if ((rc = dev.upload(&db.win_hap_off, b->win_hap_off, (size_t)W + 1))) return rc;
    if ((rc = dev.upload(&db.win_read_off, b->win_read_off, (size_t)W + 1))) return rc;
    if ((rc = dev.upload(&db.win_pair_off, (const int64_t *)pair_off.data(), pair_off.size()))) return rc;
    const int64_t *hh_dev = nullptr;
    const double *ll_dev = nullptr;
    double *out_dev = nullptr;
    if ((rc = dev.upload(&hh_dev, (const int64_t *)hh_off.data(), hh_off.size()))) return rc;
    if ((rc = dev.upload(&ll_dev, ll_host, (size_t)sz.n_pairs))) return rc;
    if ((rc = dev.alloc(&out_dev, (size_t)hh_off[W]))) return rc;
    rc = dd_pair_sums_device(&db, hh_dev, hh_off[W], ll_dev, out_dev, nullptr);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out_host, out_dev, (size_t)hh_off[W] * sizeof(double), hipMemcpyDeviceToHost));
    return DD_SUCCESS;
}
int dd_compute_likelihoods(const dd_params *p, const dd_batch *b, dd_result *r, int device)
{
    return compute_likelihoods_impl(MODEL_FBMAXERR, p, b, r, device);
}
int dd_compute_likelihoods_ex(const dd_params *p, const dd_batch *b, dd_result *r, int device, uint32_t options)
{
    if (options & ~DD_OPT_LONG_WINDOWS) return fail(DD_ERR_INVALID, "unknown option bits");
    return compute_likelihoods_impl(MODEL_FBMAXERR, p, b, r, device, options);
}
int dd_compute_likelihoods_cigars(const dd_params *p, const dd_batch *b, dd_result *r, const int32_t *hap_ref_pos, const uint8_t *hap_aligned,
                                  const dd_cigar_result *cig, int ops_cap, int device, uint32_t options)
{
    if (options & ~DD_OPT_LONG_WINDOWS) return fail(DD_ERR_INVALID, "unknown option bits");
    if (!hap_ref_pos) return fail(DD_ERR_INVALID, "dd_compute_likelihoods_cigars: hap_ref_pos is required (Haplotype::refHpos per haplotype base)");
    if (ops_cap < 1) return fail(DD_ERR_INVALID, "dd_compute_likelihoods_cigars: ops_cap must be at least 1");
    if (!cig || !cig->n_ops || !cig->ops || !cig->ref_off || !cig->status)
        return fail(DD_ERR_INVALID, "dd_compute_likelihoods_cigars: every array of dd_cigar_result is required");
    const CigarRequest cg = {hap_ref_pos, hap_aligned, *cig, ops_cap, nullptr};
    return compute_likelihoods_impl(MODEL_FBMAXERR, p, b, r, device, options, &cg);
}
int dd_compute_likelihoods_realign(const dd_params *p, const dd_batch *b, dd_result *r, int mode, const int32_t *win_hap_pair,
                                   const int32_t *hap_n_indels, const int32_t *hap_ref_pos, const uint8_t *hap_aligned,
                                   const dd_realign_result *out, int ops_cap, int device, uint32_t options)
{
    if (options & ~DD_OPT_LONG_WINDOWS) return fail(DD_ERR_INVALID, "unknown option bits");
    if (mode != DD_REALIGN_FIRST_MAX && mode != DD_REALIGN_PAIR) return fail(DD_ERR_INVALID, "dd_compute_likelihoods_realign: unknown mode");
    if (mode == DD_REALIGN_PAIR && (!win_hap_pair || !hap_n_indels))
        return fail(DD_ERR_INVALID, "dd_compute_likelihoods_realign: DD_REALIGN_PAIR needs win_hap_pair and hap_n_indels");
    if (!hap_ref_pos) return fail(DD_ERR_INVALID, "dd_compute_likelihoods_realign: hap_ref_pos is required (Haplotype::refHpos per haplotype base)");
    if (ops_cap < 1) return fail(DD_ERR_INVALID, "dd_compute_likelihoods_realign: ops_cap must be at least 1");
    if (!out || !out->hap || !out->status || !out->n_ops || !out->ops || !out->ref_off)
        return fail(DD_ERR_INVALID, "dd_compute_likelihoods_realign: every array of dd_realign_result is required");
    const RealignRequest rl = {mode, win_hap_pair, hap_n_indels, *out};
    dd_cigar_result none;
    memset(&none, 0, sizeof(none));
    const CigarRequest cg = {hap_ref_pos, hap_aligned, none, ops_cap, &rl};
    return compute_likelihoods_impl(MODEL_FBMAXERR, p, b, r, device, options, &cg);
}
int dd_compute_likelihoods_faster(const dd_params *p, const dd_batch *b, dd_result *r, int device)
{
    return compute_likelihoods_impl(MODEL_S, p, b, r, device);
}
int dd_compute_likelihoods_faster_ex(const dd_params *p, const dd_batch *b, dd_result *r, int device, uint32_t options)
{
    if (options & ~DD_OPT_LONG_WINDOWS_FASTER) return fail(DD_ERR_INVALID, "unknown option bits");
    return compute_likelihoods_impl(MODEL_S, p, b, r, device, options);
}
int dd_compute_likelihoods_multi(const dd_params *p, const dd_batch *b, dd_result *r, const int *devices, int n_devices)
{
    return compute_multi(MODEL_FBMAXERR, p, b, r, devices, n_devices);
}
int dd_compute_likelihoods_faster_multi(const dd_params *p, const dd_batch *b, dd_result *r, const int *devices, int n_devices)
{
    return compute_multi(MODEL_S, p, b, r, devices, n_devices);
}
} // extern "C"
