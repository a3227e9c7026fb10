// launch.cpp — the device-pointer launchers of the C ABI: the main and --faster kernels (shaped by plan.cpp's shape_launch / shape_fast: this
// file checks, fills the arguments and enqueues), the two long-window paths, the CIGAR and realign launches, the genotype kernels; the launch
// logs and this thread's last launch shape.
#include "capi_internal.h"

namespace ddh {
// What this host thread launched last (main model or --faster): dd_last_launch and dd_kernel_name describe it.  Per host thread, like the
// cache and the error string.
static thread_local LaunchShape g_last_shape;

// Launch log of the last dd_launch_device / dd_compute_likelihoods call on this host thread (dd_launch_log): one record per main-model
// kernel launch.  With DD_LAUNCH_TIMING=1 (diagnostics) every launch is bracketed by HIP events and its duration is filled in when the
// log is read (dd_launch_log synchronises on them).
struct LaunchRec {
    int32_t v[DD_LAUNCH_LOG_FIELDS];
    hipEvent_t e0 = nullptr, e1 = nullptr;
};
static thread_local std::vector<LaunchRec> g_launch_log;
void launch_log_clear()
{
    for (auto &r : g_launch_log) {
        if (r.e0) (void)hipEventDestroy(r.e0);
        if (r.e1) (void)hipEventDestroy(r.e1);
    }
    g_launch_log.clear();
}

#ifdef DD_STAMPS
static unsigned long long *g_dbg = nullptr;
extern "C" void dd_debug_set_stamp_buffer(void *p) { g_dbg = static_cast<unsigned long long *>(p); }   // (C linkage: the namespace does not enter its name)
#endif

// The fields KernelArgs, LongArgs and FLArgs name alike, from the batch, the parameters and the result block; what only some of them have
// (read_flags, sym_lut, hap_window, the skip / class bytes, mate arrays, D, bMid) stays with the caller.
template <class Args> static void fill_batch_args(Args &A, const dd_params *p, const dd_device_batch *b, const dd_result *r)
{
    A.n_windows = b->n_windows;
    A.win_hap_off = b->win_hap_off; A.win_read_off = b->win_read_off; A.win_hap_start = b->win_hap_start;
    A.hap_seq_off = b->hap_seq_off; A.hap_seq = b->hap_seq; A.hap_var_off = b->hap_var_off; A.hap_var = b->hap_var; A.hap_var_flank = b->hap_var_flank;
    A.read_seq_off = b->read_seq_off; A.read_seq = b->read_seq; A.read_qidx = b->read_qidx; A.read_mqidx = b->read_mqidx;
    A.read_start = b->read_start;
    A.win_pair_off = b->win_pair_off; A.win_hpos_off = b->win_hpos_off; A.win_varcov_off = b->win_varcov_off;
    A.tables = b->tables;
    A.out = *r;
    A.maxLengthDel = p->maxLengthDel; A.padCover = p->padCover; A.maxMismatch = p->maxMismatch;
}

// mapUnmappedReads: the mate arrays and library log tables of the insert-size prior, checked and handed to a main-model kernel
// (the --faster model has no such prior)
template <class Args> static int fill_mate_args(Args &A, const dd_device_batch *b)
{
    if (!b->read_mate_pos || !b->read_mate_len || !b->read_lib || !b->lib_off || !b->lib_logprob || !b->lib_log95)
        return fail(DD_ERR_INVALID, "mapUnmappedReads needs the mate arrays and the library log tables");
    A.read_mate_pos = b->read_mate_pos; A.read_mate_len = b->read_mate_len; A.read_lib = b->read_lib;
    A.lib_off = b->lib_off; A.lib_logprob = b->lib_logprob; A.lib_log95 = b->lib_log95;
    return DD_SUCCESS;
}

// Check, fill the arguments from the batch, shape the launch (plan.cpp: every decision is shape_launch's / shape_fast's), copy the shape
// into the arguments, enqueue.
int launch_range(Model model, const dd_params *p, const dd_device_batch *b, const dd_result *r, void *workspace, size_t workspace_bytes,
                 void *stream, int hap_begin, int hap_end, int read_begin, int read_end, bool overlapping_chunks, const LenClass *lc, uint32_t options)
{
    // DD_OPT_WIDE_DELETIONS lifts the parameter check for the --faster model alone: maxLengthDel is only a size check there
    int rc = check_params(p, model == MODEL_S ? options : 0);
    if (rc) return rc;
    if (!b || !r || !r->ll || !r->status) return fail(DD_ERR_INVALID, "ll and status outputs are required");
    if (b->n_haps <= 0 || b->n_reads <= 0) return DD_SUCCESS;
    if (b->max_hap_len < 1 || b->max_hap_len > DD_MAX_HAP_LEN) return fail(DD_ERR_UNSUPPORTED, "haplotype length outside [1,766]");
    if (b->max_read_len < 1 || b->max_read_len > DD_MAX_READ_LEN) return fail(DD_ERR_UNSUPPORTED, "read length outside [1,1024]");
    if (model == MODEL_S) lc = nullptr;         // the --faster model has no launch classes
    const Switches sw = read_switches();
    ddk::KernelArgs A;
    memset(&A, 0, sizeof(A));
    fill_batch_args(A, p, b, r);
    A.n_haps = b->n_haps; A.n_reads = b->n_reads;
    A.read_flags = b->read_flags; A.hap_window = b->hap_window; A.sym_lut = b->sym_lut; A.win_skip = b->win_skip;
    if (p->mapUnmappedReads && model == MODEL_FBMAXERR && (rc = fill_mate_args(A, b))) return rc;
#ifdef DD_STAMPS
    A.dbg = g_dbg;
#endif
    A.always_ro = sw.always_ro ? 1 : 0;
    A.D = p->maxLengthDel + 1; A.bMid = p->bMid;
    A.hap_list = lc ? lc->hap_list : nullptr;
    A.len_min = lc ? lc->min_read_len : 0;
    A.len_max = lc ? lc->max_read_len : 0x7fffffff;
    if (hap_end < 0) { read_begin = 0; read_end = b->n_reads; }
    A.read_begin = read_begin; A.read_end = read_end;

    LaunchAsk ask;
    ask.p = p;
    ask.n_windows = b->n_windows; ask.n_haps = b->n_haps; ask.n_reads = b->n_reads; ask.max_hap_len = b->max_hap_len; ask.max_read_len = b->max_read_len;
    ask.n_qual = b->n_qual; ask.max_window_reads = b->max_window_reads;
    ask.hap_begin = hap_begin; ask.hap_end = hap_end;
    ask.workspace_bytes = workspace ? workspace_bytes : 0;
    ask.overlapping_chunks = overlapping_chunks;
    if (lc) { ask.has_class = true; ask.cls = *lc; ask.cls.listed = lc->hap_list != nullptr; }
    LaunchShape s;
    if ((rc = model == MODEL_S ? shape_fast(sw, ask, s, A) : shape_launch(sw, ask, s, A))) return rc;
    A.n_split = (int32_t)s.split; A.reads_per_wave = s.reads_per_wave;
    A.item_begin = s.item_begin; A.n_items = s.n_items;

    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool want_onhap = r->onHap && r->offHapHMQ;
    if (model == MODEL_S) {
        A.n_qual = b->n_qual;
        A.fast_groups = s.groups;
        if (s.grid > 0) {
            g_last_shape = s;
            HIP_TRY(ddk::launch_faster(A, (unsigned)s.grid, s.waves, s.lds, st));
        }
        if (want_onhap) HIP_TRY(ddk::launch_onhap(A, st));
        return DD_SUCCESS;
    }
    if (s.pl.gbt) {
        A.bt_scratch = static_cast<unsigned char *>(workspace) + s.scratch_off;
        A.bt_rows = s.bt_rows;
        A.bt_wave_bytes = s.bt_wave_bytes;
    }
    if (s.grid <= 0) {
        if (want_onhap && lc && lc->run_onhap) HIP_TRY(ddk::launch_onhap(A, st));
        return DD_SUCCESS;
    }
    if (s.use_counter) {
        A.work_counter = static_cast<int32_t *>(workspace);
        HIP_TRY(hipMemsetAsync(workspace, 0, 4, st));
    }
    g_last_shape = s;
    LaunchRec rec;
    shape_log_record(s, rec.v);
    static const bool timing = getenv("DD_LAUNCH_TIMING") != nullptr;
    if (timing) { HIP_TRY(hipEventCreate(&rec.e0)); HIP_TRY(hipEventCreate(&rec.e1)); HIP_TRY(hipEventRecord(rec.e0, st)); }
    HIP_TRY(ddk::launch_hmm(s.pl.K, s.pl.Dt, s.pl.gbt, s.build, A, (unsigned)s.grid, s.waves, s.lds, st));
    if (timing) HIP_TRY(hipEventRecord(rec.e1, st));
    g_launch_log.push_back(rec);
    if (want_onhap && (!lc || lc->run_onhap)) HIP_TRY(ddk::launch_onhap(A, st));
    return DD_SUCCESS;
}

LenClass len_class_of(const dd_launch_class &L, const int32_t *class_list, bool run_onhap)
{
    LenClass lc;
    lc.hap_list = class_list + L.list_off; lc.listed = true; lc.list_begin = 0; lc.list_end = L.list_len;
    lc.max_hap_len = L.max_hap_len; lc.min_read_len = L.min_read_len; lc.max_read_len = L.max_read_len;
    lc.max_window_reads = L.max_window_reads; lc.avg_window_reads = L.avg_window_reads; lc.avg_read_len = L.avg_read_len;
    lc.run_onhap = run_onhap;
    return lc;
}

// ---------------- device-side getCIGAR (cigar_kernel.hip) and realigned reads (realign_kernel.hip) ----------------
// What the two launches share, behind the checks of their own arguments: the rest of the front checks in their order, then the batch's
// offset arrays and the alignment inputs into C.  every_output: no array of the result block is missing; nothing_to_do: an empty batch or
// range.  1: nothing to do, 0: go on, < 0: error (its text starts with `who`).
static int cigar_front(const char *who, const char *result_type, ddc::CigarArgs &C, const dd_device_batch *b, const int16_t *hpos,
                       const int32_t *status, const int32_t *hap_ref_pos, const uint8_t *hap_aligned, int ops_cap, bool every_output, bool nothing_to_do)
{
    auto bad = [who](const std::string &what) { return fail(DD_ERR_INVALID, std::string(who) + ": " + what); };
    if (!hap_ref_pos) return bad("hap_ref_pos is required (Haplotype::refHpos per haplotype base)");
    if (ops_cap < 1) return bad("ops_cap must be at least 1");
    if (!every_output) return bad(std::string("every array of ") + result_type + " is required");
    if (nothing_to_do) return 1;
    if (!b->win_hap_off || !b->win_read_off || !b->hap_seq_off || !b->read_seq_off || !b->win_pair_off || !b->win_hpos_off)
        return bad("the batch lacks an offset array");
    C.n_windows = b->n_windows;
    C.win_hap_off = b->win_hap_off; C.win_read_off = b->win_read_off; C.hap_seq_off = b->hap_seq_off; C.read_seq_off = b->read_seq_off;
    C.win_pair_off = b->win_pair_off; C.win_hpos_off = b->win_hpos_off;
    C.hpos = hpos; C.pair_status = status; C.hap_ref_pos = hap_ref_pos; C.hap_aligned = hap_aligned;
    C.ops_cap = ops_cap;
    return 0;
}

int launch_cigars_range(const dd_device_batch *b, const int16_t *hpos_dev, const int32_t *status_dev, const int32_t *hap_ref_pos_dev,
                        const uint8_t *hap_aligned_dev, const dd_cigar_result *out_dev, int ops_cap, void *stream, int64_t pair_begin,
                        int64_t pair_end)
{
    if (!b || !hpos_dev || !out_dev) return fail(DD_ERR_INVALID, "dd_cigars_device: null batch, hpos or output block");
    ddc::CigarArgs A;
    memset(&A, 0, sizeof(A));
    const int rc = cigar_front("dd_cigars_device", "dd_cigar_result", A, b, hpos_dev, status_dev, hap_ref_pos_dev, hap_aligned_dev, ops_cap,
                               out_dev->n_ops && out_dev->ops && out_dev->ref_off && out_dev->status,
                               b->n_windows <= 0 || b->n_haps <= 0 || b->n_reads <= 0 || (pair_end >= 0 && pair_end <= pair_begin));
    if (rc) return rc < 0 ? rc : DD_SUCCESS;
    A.pair_begin = pair_begin; A.pair_end = pair_end;
    A.out = *out_dev;
    A.max_pairs = pair_end >= 0 ? pair_end - pair_begin : (int64_t)b->n_haps * b->n_reads;
    HIP_TRY(ddc::launch_cigars(A, static_cast<hipStream_t>(stream)));
    return DD_SUCCESS;
}

int launch_realign_range(const dd_device_batch *b, const RealignInputs &in, const dd_realign_result *out_dev, int ops_cap, void *stream,
                         int read_begin, int read_end)
{
    if (!b || !in.ll || !in.hpos || !out_dev) return fail(DD_ERR_INVALID, "dd_realign_device: null batch, ll, hpos or output block");
    if (in.mode != DD_REALIGN_FIRST_MAX && in.mode != DD_REALIGN_PAIR) return fail(DD_ERR_INVALID, "dd_realign_device: unknown mode");
    if (in.mode == DD_REALIGN_PAIR && (!in.win_hap_pair || !in.hap_n_indels))
        return fail(DD_ERR_INVALID, "dd_realign_device: DD_REALIGN_PAIR needs win_hap_pair and hap_n_indels");
    if (read_end < 0) read_end = b->n_reads;
    ddc::RealignArgs A;
    memset(&A, 0, sizeof(A));
    const int rc = cigar_front("dd_realign_device", "dd_realign_result", A.cig, b, in.hpos, in.status, in.hap_ref_pos, in.hap_aligned, ops_cap,
                               out_dev->hap && out_dev->status && out_dev->n_ops && out_dev->ops && out_dev->ref_off,
                               b->n_windows <= 0 || read_end <= read_begin);      // (reads of windows without haplotypes are still marked)
    if (rc) return rc < 0 ? rc : DD_SUCCESS;
    A.cig.out.n_ops = out_dev->n_ops; A.cig.out.ops = out_dev->ops; A.cig.out.ref_off = out_dev->ref_off; A.cig.out.status = out_dev->status;
    A.mode = in.mode; A.read_begin = read_begin; A.read_end = read_end;
    A.ll = in.ll; A.on_hap = in.on_hap; A.win_hap_pair = in.win_hap_pair; A.hap_n_indels = in.hap_n_indels; A.hap = out_dev->hap;
    HIP_TRY(ddc::launch_realign(A, static_cast<hipStream_t>(stream)));
    return DD_SUCCESS;
}

// ---------------- long windows: what the two long paths share (long_kernel.hip for the main model, faster_long_kernel.hip for --faster) ----------------
// The front checks of a long launch.  1: nothing to do (empty batch or range), 0: go on, < 0: error.
static int long_front_checks(const LongPath &lp, const dd_params *p, const dd_device_batch *b, const dd_result *r, int w_begin, int w_end,
                             uint32_t options = 0)
{
    int rc = check_params(p, options);
    if (rc) return rc;
    if (!b || !r || !r->ll || !r->status) return fail(DD_ERR_INVALID, "ll and status outputs are required");
    if (b->long_max_hap_len <= 0 || b->long_max_read_len <= 0 || b->n_haps <= 0 || b->n_reads <= 0 || w_end <= w_begin) return 1;
    if (!b->win_skip) return fail(DD_ERR_INVALID, std::string(lp.name) + ": win_skip must hold dd_screen_windows_ex's classes");
    return 0;
}

// The workspace check and the fields LongArgs and FLArgs name alike; the model's own (read_flags, sym_lut, mate / library arrays, D, bMid) stay with the caller.
// ws_bytes: what the plan needs; ws_fn: the function that says so (NULL: the path's).  stats: the caller's device words, or NULL for the
// ones in the workspace header.
template <class Args>
static int long_fill_args(const LongPath &lp, Args &A, const dd_params *p, const dd_device_batch *b, const dd_result *r, void *workspace,
                          size_t workspace_bytes, uint64_t ws_bytes, int w_begin, int w_end, int read_begin, int read_end, unsigned long long *stats,
                          const char *ws_fn = nullptr)
{
    if (!workspace || workspace_bytes < ws_bytes)
        return fail(DD_ERR_INVALID, std::string("workspace too small for the ") + lp.name + ": allocate " + (ws_fn ? ws_fn : lp.ws_fn) + "() bytes");
    fill_batch_args(A, p, b, r);
    A.w_begin = w_begin; A.w_end = w_end; A.read_begin = read_begin; A.read_end = read_end;
    A.win_class = b->win_skip;
    A.ws = static_cast<unsigned char *>(workspace);
    A.stats = stats ? stats : reinterpret_cast<unsigned long long *>(A.ws + DD_LWS_HDR_STATS);
    return DD_SUCCESS;
}

// v: the record's fields, those of the stats words still -1
static void long_log_push(LongPath &lp, const int64_t (&v)[DD_LONG_LOG_FIELDS], const unsigned long long *stats, hipStream_t st)
{
    LongRec rec;
    memcpy(rec.v, v, sizeof(v));
    rec.stats = stats;
    rec.stream = st;
    lp.log.push_back(rec);
}

// the records of a path's log; the stats words of a launch are read back (after its stream has drained) the first time they are asked for
static int long_read_log(LongPath &lp, int64_t *out, int max_records)
{
    const int n = (int)lp.log.size();
    for (int i = 0; i < n && i < max_records && out; i++) {
        LongRec &r = lp.log[(size_t)i];
        if (r.stats && r.v[1] < 0) {
            unsigned long long st[4] = {0, 0, 0, 0};
            if (hipStreamSynchronize(r.stream) == hipSuccess && hipMemcpy(st, r.stats, (size_t)lp.n_stats * sizeof(st[0]), hipMemcpyDeviceToHost) == hipSuccess) {
                for (int k = 0; k < lp.n_stats; k++)
                    if (lp.stat_field[k] >= 0) r.v[lp.stat_field[k]] = (int64_t)st[k];
            } else {
                (void)hipGetLastError();
            }
        }
        memcpy(out + (size_t)i * DD_LONG_LOG_FIELDS, r.v, sizeof(r.v));
    }
    return n;
}

// ---------------- long windows of the main model (long_kernel.hip) ----------------
// one long launch over the windows [w_begin, w_end) (their reads: [read_begin, read_end)); stats: device words the kernel counts into.
// options with DD_OPT_WIDE_DELETIONS and maxLengthDel > 31: the wide build, which also writes the placeholders of the other windows of the
// range and onHap of all its reads (there is no main launch for these parameters).
static int launch_long_range(const dd_params *p, const dd_device_batch *b, const dd_result *r, void *workspace, size_t workspace_bytes,
                             void *stream, int w_begin, int w_end, int read_begin, int read_end, unsigned long long *stats, uint32_t options)
{
    int rc = long_front_checks(g_long, p, b, r, w_begin, w_end, options);
    if (rc < 0) return rc;
    const bool wide = wide_on(p, options);
    ddl::LongArgs A;
    memset(&A, 0, sizeof(A));
    if (rc && wide && b->n_haps > 0 && b->n_reads > 0 && w_end > w_begin) {
        // no long window in the batch: placeholders and onHap are still this launch's to write
        if (!b->win_skip) return fail(DD_ERR_INVALID, "long path: win_skip must hold dd_screen_windows_ex's classes");
        fill_batch_args(A, p, b, r);
        A.w_begin = w_begin; A.w_end = w_end; A.read_begin = read_begin; A.read_end = read_end;
        A.win_class = b->win_skip;
        HIP_TRY(ddl::launch_wide_tail(A, r->onHap && r->offHapHMQ, static_cast<hipStream_t>(stream)));
        return DD_SUCCESS;
    }
    if (rc) return DD_SUCCESS;
    LongPlan lp;
    if ((rc = long_plan(b->n_windows, b->long_max_hap_len, b->long_max_read_len, b->n_qual, lp, A, wide))) return rc;
    if ((rc = long_fill_args(g_long, A, p, b, r, workspace, workspace_bytes, lp.ws_bytes, w_begin, w_end, read_begin, read_end, stats,
                             wide ? "dd_workspace_bytes_wide" : nullptr))) return rc;
    A.read_flags = b->read_flags; A.sym_lut = b->sym_lut;
    if (p->mapUnmappedReads && (rc = fill_mate_args(A, b))) return rc;
    A.D = p->maxLengthDel + 1; A.bMid = p->bMid;
    A.max_read_len = b->long_max_read_len;
    A.off_lpoff = lp.off_lpoff; A.off_tiles = lp.off_tiles; A.tile_bytes = lp.tile_bytes; A.stash_off = lp.stash_off;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool onhap = r->onHap && r->offHapHMQ;
    HIP_TRY(ddl::launch_long(lp.K, wide, A, lp.grid, lp.lds, onhap, st));
    const int64_t v[DD_LONG_LOG_FIELDS] = {(int64_t)lp.grid, -1, -1, (int64_t)lp.ws_bytes, lp.K | (wide ? DD_LONG_LOG_WIDE : 0), b->long_max_hap_len,
                                           b->long_max_read_len, (int64_t)lp.lds};
    long_log_push(g_long, v, A.stats, st);
    return DD_SUCCESS;
}

// ---------------- long windows of the --faster model (faster_long_kernel.hip) ----------------
// one launch over the windows [w_begin, w_end) (their reads: [read_begin, read_end)); stats: 4 device words the kernel counts into;
// options: DD_OPT_WIDE_DELETIONS lifts the parameter check (maxLengthDel is only a size check in this model)
static int launch_faster_long_range(const dd_params *p, const dd_device_batch *b, const dd_result *r, void *workspace, size_t workspace_bytes,
                                        void *stream, int w_begin, int w_end, int read_begin, int read_end, unsigned long long *stats, uint32_t options)
{
    int rc = long_front_checks(g_flong, p, b, r, w_begin, w_end, options);
    if (rc) return rc < 0 ? rc : DD_SUCCESS;
    ddf::FLArgs A;
    memset(&A, 0, sizeof(A));
    FLPlan fp;
    if ((rc = fl_plan(b, fp, A))) return rc;
    if ((rc = long_fill_args(g_flong, A, p, b, r, workspace, workspace_bytes, fp.ws_bytes, w_begin, w_end, read_begin, read_end, stats))) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(ddf::launch_faster_long(A, fp.grid, fp.lds, r->onHap && r->offHapHMQ, st));
    const int64_t v[DD_FASTER_LONG_LOG_FIELDS] = {(int64_t)fp.grid, -1, -1, (int64_t)fp.ws_bytes, -1, b->long_max_hap_len, b->long_max_read_len, (int64_t)fp.lds};
    long_log_push(g_flong, v, A.stats, st);
    return DD_SUCCESS;
}

// stats: {pairs, most pairs of one workgroup} / {pairs, most pairs of one workgroup, most items of one workgroup, 0}
thread_local LongPath g_long = {"long path", "dd_workspace_bytes_long", 2, {1, 2, -1, -1}, launch_long_range, dd_workspace_bytes_long, {}};
thread_local LongPath g_flong = {"--faster long path", "dd_workspace_bytes_faster_long", 4, {1, 2, 4, -1}, launch_faster_long_range,
                                        dd_workspace_bytes_faster_long, {}};
} // namespace ddh
using namespace ddh;
extern "C" {
const char *dd_kernel_name(void)
{   // the kernel this host thread launched last
    static thread_local char name[64];
    shape_kernel_name(g_last_shape, name, sizeof(name));
    return name;
}

void dd_last_launch(int32_t out[8]) { shape_last_launch(g_last_shape, out); }

int dd_launch_log(int32_t *out, int max_records)
{   // see include/dindel_hmm.h
    const int n = (int)g_launch_log.size();
    for (int i = 0; i < n && i < max_records && out; i++) {
        LaunchRec &r = g_launch_log[(size_t)i];
        if (r.e0 && r.e1) {
            float ms = 0.f;
            if (hipEventSynchronize(r.e1) == hipSuccess && hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) r.v[15] = (int32_t)(ms * 1000.f + 0.5f);
        }
        memcpy(out + (size_t)i * DD_LAUNCH_LOG_FIELDS, r.v, sizeof(r.v));
    }
    return n;
}

int dd_launch_device_long(const dd_params *p, const dd_device_batch *b, const dd_result *r, void *workspace, size_t workspace_bytes, void *stream)
{
    g_long.log.clear();
    if (!b) return fail(DD_ERR_INVALID, "null batch");
    return launch_long_range(p, b, r, workspace, workspace_bytes, stream, 0, b->n_windows, 0, b->n_reads, nullptr, 0);
}
int dd_launch_device_wide(const dd_params *p, const dd_device_batch *b, const dd_result *r, void *workspace, size_t workspace_bytes, void *stream)
{
    g_long.log.clear();
    if (!b) return fail(DD_ERR_INVALID, "null batch");
    return launch_long_range(p, b, r, workspace, workspace_bytes, stream, 0, b->n_windows, 0, b->n_reads, nullptr, DD_OPT_WIDE_DELETIONS);
}
int dd_long_launch_log(int64_t *out, int max_records) { return long_read_log(g_long, out, max_records); }   // see include/dindel_hmm.h

int dd_launch_device_faster_long(const dd_params *p, const dd_device_batch *b, const dd_result *r, void *workspace, size_t workspace_bytes, void *stream)
{
    g_flong.log.clear();
    if (!b) return fail(DD_ERR_INVALID, "null batch");
    return launch_faster_long_range(p, b, r, workspace, workspace_bytes, stream, 0, b->n_windows, 0, b->n_reads, nullptr, 0);
}
int dd_faster_long_launch_log(int64_t *out, int max_records) { return long_read_log(g_flong, out, max_records); }   // see include/dindel_hmm.h

int dd_launch_device(const dd_params *p, const dd_device_batch *b, const dd_result *r, void *workspace, size_t workspace_bytes, void *stream)
{
    launch_log_clear();
    if (b && b->classes && b->hap_class_list && b->classes->n_launches > 1) {
        // ragged batch: one launch per (lane tiling, read-length interval) that has work, onHap once at the end
        const dd_length_classes *C = b->classes;
        for (int i = 0; i < C->n_launches; i++) {
            const LenClass lc = len_class_of(C->launch[i], b->hap_class_list, i == C->n_launches - 1);
            const int rc = launch_range(MODEL_FBMAXERR, p, b, r, workspace, workspace_bytes, stream, 0, b->n_haps, 0, b->n_reads, false, &lc);
            if (rc) return rc;
        }
        return DD_SUCCESS;
    }
    return launch_range(MODEL_FBMAXERR, p, b, r, workspace, workspace_bytes, stream, 0, -1, 0, 0, false);
}
int dd_launch_device_faster(const dd_params *p, const dd_device_batch *b, const dd_result *r, void *stream)
{
    return launch_range(MODEL_S, p, b, r, nullptr, 0, stream, 0, -1, 0, 0, false);
}
int dd_launch_device_faster_ex(const dd_params *p, const dd_device_batch *b, const dd_result *r, void *stream, uint32_t options)
{
    if (options & ~DD_OPT_WIDE_DELETIONS) return fail(DD_ERR_INVALID, "dd_launch_device_faster_ex: unknown option bits (0 or DD_OPT_WIDE_DELETIONS)");
    return launch_range(MODEL_S, p, b, r, nullptr, 0, stream, 0, -1, 0, 0, false, nullptr, options);
}

int dd_cigars_device(const dd_device_batch *b, const int16_t *hpos_dev, const int32_t *status_dev, const int32_t *hap_ref_pos_dev,
                     const uint8_t *hap_aligned_dev, const dd_cigar_result *out_dev, int ops_cap, void *stream)
{   // the whole batch: the pair count is win_pair_off[n_windows], a device array, so the kernel reads its own bound there
    return launch_cigars_range(b, hpos_dev, status_dev, hap_ref_pos_dev, hap_aligned_dev, out_dev, ops_cap, stream, 0, -1);
}

int dd_realign_device(const dd_device_batch *b, int mode, const double *ll_dev, const uint8_t *on_hap_dev,
                      const int32_t *win_hap_pair_dev, const int32_t *hap_n_indels_dev,
                      const int16_t *hpos_dev, const int32_t *status_dev, const int32_t *hap_ref_pos_dev,
                      const uint8_t *hap_aligned_dev, const dd_realign_result *out_dev, int ops_cap, void *stream)
{
    const RealignInputs in = {mode, ll_dev, on_hap_dev, win_hap_pair_dev, hap_n_indels_dev, hpos_dev, status_dev, hap_ref_pos_dev, hap_aligned_dev};
    return launch_realign_range(b, in, out_dev, ops_cap, stream, 0, -1);
}

int dd_pair_sums_device(const dd_device_batch *b, const int64_t *win_hh_off_dev, int64_t n_slots,
                        const double *ll_dev, double *out_dev, void *stream)
{
    if (!b || !win_hh_off_dev || !ll_dev || !out_dev) return fail(DD_ERR_INVALID, "null argument");
    ddk::PairSumArgs A;
    A.n_windows = b->n_windows; A.n_slots = n_slots;
    A.win_hap_off = b->win_hap_off; A.win_read_off = b->win_read_off; A.win_pair_off = b->win_pair_off;
    A.win_hh_off = win_hh_off_dev; A.ll = ll_dev; A.out = out_dev;
    if ((n_slots + 3) / 4 > 0x7fffffffLL) return fail(DD_ERR_UNSUPPORTED, "batch too large for one launch");
    HIP_TRY(ddk::launch_pair_sums(A, static_cast<hipStream_t>(stream)));
    return DD_SUCCESS;
}

int dd_map_pairs_device(const dd_device_batch *b, const int64_t *win_hh_off_dev, const double *pair_sum_dev, const double *prior_dev,
                        const uint8_t *filtered_dev, const int32_t *ncand_dev, double *posterior_dev, int32_t *pairs_dev,
                        double *vals_dev, void *stream)
{
    if (!b || !win_hh_off_dev || !pair_sum_dev || !prior_dev || !filtered_dev || !ncand_dev || !pairs_dev || !vals_dev)
        return fail(DD_ERR_INVALID, "null argument");
    ddk::MapPairArgs A;
    A.n_windows = b->n_windows; A.win_hap_off = b->win_hap_off; A.win_hh_off = win_hh_off_dev;
    A.pair_sum = pair_sum_dev; A.prior = prior_dev; A.filtered = filtered_dev; A.ncand = ncand_dev;
    A.posterior = posterior_dev; A.pairs = pairs_dev; A.vals = vals_dev;
    HIP_TRY(ddk::launch_map_pairs(A, static_cast<hipStream_t>(stream)));
    return DD_SUCCESS;
}
} // extern "C"
