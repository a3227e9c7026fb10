// launch.cpp — the device-pointer launchers of the C ABI: the main and --faster kernels, the two long-window paths, the genotype kernels;
// the launch logs and the per-thread diagnostics that describe the last launch.
#include "capi_internal.h"

namespace ddh {
static thread_local int32_t g_last_launch[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // per host thread, like the cache and the error string
static thread_local char g_kernel_name[64] = "dd_hmm_kernel";
static thread_local int g_last_fold = 0;       // the last main-model launch used the FOLD build (hmm_kernel.hip)
static thread_local int g_last_G = 1;          // ... pairs per wavefront of that launch
static thread_local int g_last_occ = 0;        // ... the build variant compiled for that many waves per SIMD (0 = the build's usual occupancy)

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

static int launch_fast(const dd_params *p, const dd_device_batch *b, ddk::KernelArgs &A, void *stream, int hap_begin, int hap_end,
                       int read_begin, int read_end, bool want_onhap)
{
    (void)p;
    int waves = DD_WAVES, groups = 4;
    size_t lds = lds_layout_fast(b->max_hap_len, b->max_read_len, b->n_qual, waves, groups, A);
    if (lds > kCuLdsBytes) return fail(DD_ERR_UNSUPPORTED, "shape exceeds the LDS tile of the --faster kernel");
    A.n_qual = b->n_qual;
    A.fast_groups = groups;
    int64_t target_blocks = 1024;                 // workgroups wanted before haplotypes are split (A/B: DD_FAST_TARGET_BLOCKS)
    if (const char *e = getenv("DD_FAST_TARGET_BLOCKS")) { const long v = atol(e); if (v >= 1) target_blocks = v; }   // A/B only
    int64_t avg_reads = (b->n_reads + b->n_windows - 1) / (b->n_windows > 0 ? b->n_windows : 1);
    {   // thin windows: no more wavefronts per workgroup than the windows have groups of `groups` reads
        const int w2 = waves_for_reads((avg_reads + groups - 1) / groups, waves, 8);
        if (w2 != waves) {
            waves = w2;
            lds = (size_t)A.lds_shared_bytes + (size_t)waves * (groups < 4 ? groups + 1 : 4) * A.lds_wave_bytes;
        }
    }
    const int64_t split = pick_split(hap_end - hap_begin, (avg_reads + groups - 1) / groups, waves, target_blocks);
    if ((int64_t)b->n_haps * split > 0x7fffffffLL) return fail(DD_ERR_UNSUPPORTED, "batch too large for one launch");
    A.n_split = (int32_t)split;
    A.item_begin = (int32_t)(hap_begin * split);
    A.n_items = (int32_t)(hap_end * split);
    A.read_begin = read_begin; A.read_end = read_end;
    A.hap_list = nullptr; A.len_min = 0; A.len_max = 0x7fffffff;
    int64_t grid = (int64_t)(hap_end - hap_begin) * split;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (grid > 0) {
        g_last_launch[0] = groups; g_last_launch[1] = 0; g_last_launch[2] = waves; g_last_launch[3] = (int32_t)lds;
        g_last_launch[4] = (int32_t)grid; g_last_launch[5] = (int32_t)split; g_last_launch[6] = (int32_t)A.lds_wave_bytes; g_last_launch[7] = 0;
        HIP_TRY(ddk::launch_faster(A, (unsigned)grid, waves, lds, st));
    }
    if (want_onhap) HIP_TRY(ddk::launch_onhap(A, st));
    return DD_SUCCESS;
}

int launch_range(Model model, const dd_params *p, const dd_device_batch *b, const dd_result *r, void *workspace, size_t workspace_bytes,
                 void *stream, int hap_begin, int hap_end, int read_begin, int read_end, bool overlapping_chunks, const LenClass *lc)
{
    int rc = check_params(p);
    if (rc) return rc;
    if (!b || !r || !r->ll || !r->status) return fail(DD_ERR_INVALID, "ll and status outputs are required");
    if (b->n_haps <= 0 || b->n_reads <= 0) return DD_SUCCESS;
    if (b->max_hap_len < 1 || b->max_hap_len > DD_MAX_HAP_LEN) return fail(DD_ERR_UNSUPPORTED, "haplotype length outside [1,766]");
    if (b->max_read_len < 1 || b->max_read_len > DD_MAX_READ_LEN) return fail(DD_ERR_UNSUPPORTED, "read length outside [1,1024]");
    const int D = p->maxLengthDel + 1;
    ddk::KernelArgs A;
    memset(&A, 0, sizeof(A));
    A.n_windows = b->n_windows; A.n_haps = b->n_haps; A.n_reads = b->n_reads;
    A.win_hap_off = b->win_hap_off; A.win_read_off = b->win_read_off; A.win_hap_start = b->win_hap_start;
    A.hap_seq_off = b->hap_seq_off; A.hap_seq = b->hap_seq; A.hap_var_off = b->hap_var_off; A.hap_var = b->hap_var; A.hap_var_flank = b->hap_var_flank;
    A.read_seq_off = b->read_seq_off; A.read_seq = b->read_seq; A.read_qidx = b->read_qidx; A.read_mqidx = b->read_mqidx;
    A.read_start = b->read_start; A.read_flags = b->read_flags;
    A.hap_window = b->hap_window; A.win_pair_off = b->win_pair_off; A.win_hpos_off = b->win_hpos_off;
    A.win_varcov_off = b->win_varcov_off; A.tables = b->tables; A.sym_lut = b->sym_lut; A.win_skip = b->win_skip;
    if (p->mapUnmappedReads && model == MODEL_FBMAXERR && (rc = fill_mate_args(A, b))) return rc;
    A.out = *r;
#ifdef DD_STAMPS
    A.dbg = g_dbg;
#endif
    A.always_ro = getenv("DD_ALWAYS_RO") ? 1 : 0;
    A.D = D; A.maxLengthDel = p->maxLengthDel; A.padCover = p->padCover; A.bMid = p->bMid; A.maxMismatch = p->maxMismatch;
    if (model == MODEL_S) {
        if (hap_end < 0) { hap_begin = 0; hap_end = b->n_haps; read_begin = 0; read_end = b->n_reads; }
        return launch_fast(p, b, A, stream, hap_begin, hap_end, read_begin, read_end, r->onHap && r->offHapHMQ);
    }
    Plan pl;
    const int cls_hap = lc ? lc->max_hap_len : b->max_hap_len, cls_read = lc ? lc->max_read_len : b->max_read_len;
    rc = make_plan(p, cls_hap, cls_read, b->n_qual, pl, A);
    if (rc) return rc;
    A.hap_list = lc ? lc->hap_list : nullptr;
    A.len_min = lc ? lc->min_read_len : 0;
    A.len_max = lc ? lc->max_read_len : 0x7fffffff;
    const int K = pl.K, Dt = pl.Dt;
    int waves = pl.waves;
    size_t lds = pl.lds;
    // thin windows: a wavefront works on one read at a time, so a workgroup never needs more waves than the windows have
    // reads (tools/coverage_sweep.py: 2 reads per window ran at half the rate with idle waves in every workgroup)
    const int64_t avg_reads_w = (lc && lc->avg_window_reads > 0) ? lc->avg_window_reads : (b->n_reads + b->n_windows - 1) / (b->n_windows > 0 ? b->n_windows : 1);
    {
        const int w2 = waves_for_reads((avg_reads_w + pl.G - 1) / pl.G, waves, pl.waves_per_cu);   // a wavefront takes G reads at a time
        if (w2 != waves) {
            waves = w2;
            lds = lds_layout(K, Dt, cls_read, b->n_qual, waves, pl.gbt, pl.G, A);
        }
    }
    if (pl.gbt) {
        if (!workspace || workspace_bytes < pl.scratch_bytes + DD_WS_HEADER)
            return fail(DD_ERR_INVALID, "workspace too small for this shape: allocate dd_workspace_bytes() bytes");
        A.bt_scratch = static_cast<unsigned char *>(workspace) + DD_WS_HEADER;
        A.bt_rows = cls_read;
        A.bt_wave_bytes = (uint32_t)scratch_wave_bytes(K, Dt, pl.G, cls_read);
    }
    // enough workgroups to fill 256 CUs several times over, but keep >= 1 read per wave
    int64_t target_blocks = 4096;
    if (const char *e = getenv("DD_TARGET_BLOCKS")) { const long v = atol(e); if (v >= 1) target_blocks = v; }   // A/B only
    int64_t avg_reads = avg_reads_w;
    if (hap_end < 0) { hap_begin = 0; hap_end = b->n_haps; read_begin = 0; read_end = b->n_reads; }
    if (lc && lc->hap_list) { hap_begin = lc->list_begin; hap_end = lc->list_end; }   // positions in the class list
    // the split is chosen for the haplotypes THIS launch covers: a rare length class or a small window block must still
    // spread over the chip
    // workgroups the chip holds at once (one-shot grids; a persistent GBT grid is capped to that number below anyway)
    int64_t resident = resident_workgroups(lds, pl.waves_per_cu, waves);
    if (getenv("DD_SPLIT_NO_ROUNDS")) resident = 0;                            // A/B only: the rule before round 3
    int64_t split = pick_split(hap_end - hap_begin, (avg_reads + pl.G - 1) / pl.G, waves, target_blocks, resident);
    // Ragged windows: `split` suits a window with the average number of reads; a haplotype whose window has more gets proportionally more
    // workgroups (the kernel derives its own count from reads_per_wave), so that a 400-read window among 100-read ones does not end the
    // launch with one workgroup still at work; when the spread is wide the work of a wavefront is also capped (DD_READS_PER_WAVE, A/B).
    A.reads_per_wave = 0;
    const int max_reads = (lc && lc->max_window_reads > 0) ? lc->max_window_reads : b->max_window_reads;
    if (max_reads > 0 && max_reads * 4 > avg_reads * 5 && !getenv("DD_UNIFORM_SPLIT")) {
        const int64_t units = (avg_reads + pl.G - 1) / pl.G, max_units = (max_reads + pl.G - 1) / pl.G;
        int64_t rpw = (units + waves * split - 1) / (waves * split);
        int cap_rpw = (Dt > 7 || K >= 3) ? 24 : 12;
        if (const char *e = getenv("DD_READS_PER_WAVE")) { const int v = atoi(e); if (v >= 1) cap_rpw = v; }
        if (rpw > cap_rpw) rpw = cap_rpw;
        if (rpw < 1) rpw = 1;
        A.reads_per_wave = (int32_t)rpw;
        split = (max_units + waves * rpw - 1) / (waves * rpw);
        if (split < 1) split = 1;
    }
    A.n_split = (int32_t)split;
    if ((int64_t)b->n_haps * split > 0x7fffffffLL) return fail(DD_ERR_UNSUPPORTED, "batch too large for one launch");
    A.item_begin = (int32_t)(hap_begin * split);
    A.n_items = (int32_t)(hap_end * split);
    A.read_begin = read_begin; A.read_end = read_end;
    int64_t grid = (int64_t)(hap_end - hap_begin) * split;
    if (grid <= 0) {
        if (r->onHap && r->offHapHMQ && lc && lc->run_onhap) HIP_TRY(ddk::launch_onhap(A, static_cast<hipStream_t>(stream)));
        return DD_SUCCESS;
    }
    const int64_t n_launch_items = grid;
    if (pl.grid_cap) {
        // the scratch holds grid_cap x pl.waves back-pointer tiles; smaller workgroups (thin windows) may be more numerous
        const int64_t cap = (int64_t)pl.grid_cap * pl.waves / waves;
        if (grid > cap) grid = cap;
    }
    // More items than the chip holds workgroups: a persistent grid that draws its items from a counter.  Built for the ragged launches (items that
    // differ 20-fold in work); at the end of round 4 it turned out to be worth as much on UNIFORM batches wherever the grid was persistent
    // already — every HBM-scratch build ran a fixed stride, and the items of a uniform batch still differ by their reads' bMid: 3.42 -> 3.85e11 cells/s
    // at 130 bp, 3.34 -> 3.88e11 at 80 bp, +10-18 % on every K >= 3 tiling (profiles/r04/item_counter_uniform_ab.txt) — and +0.1-1.5 % on the
    // one-shot LDS grids (the headline build: +0.9 %), whose XCD-contiguous numbering (one L2 per window's haplotypes) it gives up.
    hipStream_t st = static_cast<hipStream_t>(stream);
    A.work_counter = nullptr;
    {
        // (Except: the chunks of the host-pointer path alternate between two streams, and a one-shot grid lets the next chunk's workgroups move in
        // while this one's drain; a chip-filling persistent grid holds its slots to the end — `dd_compute_likelihoods` with pageable pointers lost 7 %
        // that way, 23.7 -> 22.0 k windows/s at configs[1].  There the LDS builds keep their one-shot grids unless the batch is ragged.)
        const bool spread = A.reads_per_wave > 0 || (lc && lc->avg_read_len > 0 && lc->max_read_len * 4 > lc->avg_read_len * 5);
        const char *e = getenv("DD_DYNAMIC");                                 // A/B: 0 = never (one-shot LDS grids, fixed stride on scratch builds)
        const bool dynamic = e ? (e[0] == '1') : (pl.gbt || spread || !overlapping_chunks);
        if (dynamic && workspace && workspace_bytes >= DD_WS_HEADER && resident > 0 && n_launch_items > resident) {
            A.work_counter = static_cast<int32_t *>(workspace);
            HIP_TRY(hipMemsetAsync(workspace, 0, 4, st));
            if (grid > resident) grid = resident;
        }
    }
    g_last_launch[0] = K; g_last_launch[1] = Dt + (pl.gbt ? 100 : 0); g_last_launch[2] = waves; g_last_launch[3] = (int32_t)lds;
    g_last_launch[4] = (int32_t)grid; g_last_launch[5] = (int32_t)split; g_last_launch[6] = (int32_t)A.lds_wave_bytes;
    g_last_launch[7] = (int32_t)A.lds_shared_bytes;
    // the build with the end states folded into the generic candidate code (hmm_kernel.hip, FOLD): K <= 2 at D build 6 with LDS
    // back-pointers, K = 2 at D build 6 with scratch back-pointers, K = 2 at D build 11 with LDS back-pointers — and every haplotype
    // of this launch leaves position 64 K - 1 idle (numS <= 64 K - 1)
    const bool fold_build = pl.gbt ? (K == 2 && Dt == 6) : ((K <= 2 && Dt == 6) || (K == 2 && Dt == 11));     // the builds measured to gain from it
    const bool fold = pl.G == 1 && fold_build && 64 * K >= cls_hap + 3 && !getenv("DD_NO_FOLD");
    g_last_fold = fold ? 1 : 0;
    g_last_occ = (pl.gbt && pl.two_waves) ? 2 : 0;
    const int build = (fold ? DD_BUILD_FOLD : 0) | ((pl.gbt && pl.two_waves) ? DD_BUILD_TWO_WAVES : 0) | (pl.G == 2 ? DD_BUILD_HALF : 0);
    g_last_G = pl.G;
    LaunchRec rec;
    {
        const int32_t v[DD_LAUNCH_LOG_FIELDS] = {K, pl.G, Dt, pl.gbt ? 1 : 0, fold ? 1 : 0, waves, (int32_t)lds, (int32_t)grid, (int32_t)split,
                                                 hap_end - hap_begin, cls_hap, lc ? lc->min_read_len : 1, cls_read, pl.waves_per_cu, g_last_occ, -1,
                                                 A.work_counter ? 1 : 0, A.reads_per_wave};
        memcpy(rec.v, v, sizeof(v));
    }
    static const bool timing = getenv("DD_LAUNCH_TIMING") != nullptr;
    if (timing) { HIP_TRY(hipEventCreate(&rec.e0)); HIP_TRY(hipEventCreate(&rec.e1)); HIP_TRY(hipEventRecord(rec.e0, st)); }
    HIP_TRY(ddk::launch_hmm(K, Dt, pl.gbt, build, A, (unsigned)grid, waves, lds, st));
    if (timing) HIP_TRY(hipEventRecord(rec.e1, st));
    g_launch_log.push_back(rec);
    if (r->onHap && r->offHapHMQ && (!lc || lc->run_onhap)) HIP_TRY(ddk::launch_onhap(A, st));
    return DD_SUCCESS;
}

LenClass len_class_of(const dd_launch_class &L, const int32_t *class_list, bool run_onhap)
{
    LenClass lc;
    lc.hap_list = class_list + L.list_off; lc.list_begin = 0; lc.list_end = L.list_len;
    lc.max_hap_len = L.max_hap_len; lc.min_read_len = L.min_read_len; lc.max_read_len = L.max_read_len;
    lc.max_window_reads = L.max_window_reads; lc.avg_window_reads = L.avg_window_reads; lc.avg_read_len = L.avg_read_len;
    lc.run_onhap = run_onhap;
    return lc;
}

// ---------------- device-side getCIGAR (cigar_kernel.hip) ----------------
int launch_cigars_range(const dd_device_batch *b, const int16_t *hpos_dev, const int32_t *status_dev, const int32_t *hap_ref_pos_dev,
                        const uint8_t *hap_aligned_dev, const dd_cigar_result *out_dev, int ops_cap, void *stream, int64_t pair_begin,
                        int64_t pair_end)
{
    if (!b || !hpos_dev || !out_dev) return fail(DD_ERR_INVALID, "dd_cigars_device: null batch, hpos or output block");
    if (!hap_ref_pos_dev) return fail(DD_ERR_INVALID, "dd_cigars_device: hap_ref_pos is required (Haplotype::refHpos per haplotype base)");
    if (ops_cap < 1) return fail(DD_ERR_INVALID, "dd_cigars_device: ops_cap must be at least 1");
    if (!out_dev->n_ops || !out_dev->ops || !out_dev->ref_off || !out_dev->status) return fail(DD_ERR_INVALID, "dd_cigars_device: every array of dd_cigar_result is required");
    if (b->n_windows <= 0 || b->n_haps <= 0 || b->n_reads <= 0 || (pair_end >= 0 && pair_end <= pair_begin)) return DD_SUCCESS;
    if (!b->win_hap_off || !b->win_read_off || !b->hap_seq_off || !b->read_seq_off || !b->win_pair_off || !b->win_hpos_off)
        return fail(DD_ERR_INVALID, "dd_cigars_device: the batch lacks an offset array");
    ddc::CigarArgs A;
    memset(&A, 0, sizeof(A));
    A.n_windows = b->n_windows; A.pair_begin = pair_begin; A.pair_end = pair_end;
    A.win_hap_off = b->win_hap_off; A.win_read_off = b->win_read_off; A.hap_seq_off = b->hap_seq_off; A.read_seq_off = b->read_seq_off;
    A.win_pair_off = b->win_pair_off; A.win_hpos_off = b->win_hpos_off;
    A.hpos = hpos_dev; A.pair_status = status_dev; A.hap_ref_pos = hap_ref_pos_dev; A.hap_aligned = hap_aligned_dev;
    A.out = *out_dev; A.ops_cap = ops_cap;
    A.max_pairs = pair_end >= 0 ? pair_end - pair_begin : (int64_t)b->n_haps * b->n_reads;
    HIP_TRY(ddc::launch_cigars(A, static_cast<hipStream_t>(stream)));
    return DD_SUCCESS;
}

// ---------------- realigned reads (realign_kernel.hip) ----------------
int launch_realign_range(const dd_device_batch *b, const RealignInputs &in, const dd_realign_result *out_dev, int ops_cap, void *stream,
                         int read_begin, int read_end)
{
    if (!b || !in.ll || !in.hpos || !out_dev) return fail(DD_ERR_INVALID, "dd_realign_device: null batch, ll, hpos or output block");
    if (in.mode != DD_REALIGN_FIRST_MAX && in.mode != DD_REALIGN_PAIR) return fail(DD_ERR_INVALID, "dd_realign_device: unknown mode");
    if (in.mode == DD_REALIGN_PAIR && (!in.win_hap_pair || !in.hap_n_indels))
        return fail(DD_ERR_INVALID, "dd_realign_device: DD_REALIGN_PAIR needs win_hap_pair and hap_n_indels");
    if (!in.hap_ref_pos) return fail(DD_ERR_INVALID, "dd_realign_device: hap_ref_pos is required (Haplotype::refHpos per haplotype base)");
    if (ops_cap < 1) return fail(DD_ERR_INVALID, "dd_realign_device: ops_cap must be at least 1");
    if (!out_dev->hap || !out_dev->status || !out_dev->n_ops || !out_dev->ops || !out_dev->ref_off)
        return fail(DD_ERR_INVALID, "dd_realign_device: every array of dd_realign_result is required");
    if (read_end < 0) read_end = b->n_reads;
    if (b->n_windows <= 0 || read_end <= read_begin) return DD_SUCCESS;      // (reads of windows without haplotypes are still marked)
    if (!b->win_hap_off || !b->win_read_off || !b->hap_seq_off || !b->read_seq_off || !b->win_pair_off || !b->win_hpos_off)
        return fail(DD_ERR_INVALID, "dd_realign_device: the batch lacks an offset array");
    ddc::RealignArgs A;
    memset(&A, 0, sizeof(A));
    ddc::CigarArgs &C = A.cig;
    C.n_windows = b->n_windows;
    C.win_hap_off = b->win_hap_off; C.win_read_off = b->win_read_off; C.hap_seq_off = b->hap_seq_off; C.read_seq_off = b->read_seq_off;
    C.win_pair_off = b->win_pair_off; C.win_hpos_off = b->win_hpos_off;
    C.hpos = in.hpos; C.pair_status = in.status; C.hap_ref_pos = in.hap_ref_pos; C.hap_aligned = in.hap_aligned;
    C.out.n_ops = out_dev->n_ops; C.out.ops = out_dev->ops; C.out.ref_off = out_dev->ref_off; C.out.status = out_dev->status;
    C.ops_cap = ops_cap;
    A.mode = in.mode; A.read_begin = read_begin; A.read_end = read_end;
    A.ll = in.ll; A.on_hap = in.on_hap; A.win_hap_pair = in.win_hap_pair; A.hap_n_indels = in.hap_n_indels; A.hap = out_dev->hap;
    HIP_TRY(ddc::launch_realign(A, static_cast<hipStream_t>(stream)));
    return DD_SUCCESS;
}

// ---------------- long windows: what the two long paths share (long_kernel.hip for the main model, faster_long_kernel.hip for --faster) ----------------
// The front checks of a long launch.  1: nothing to do (empty batch or range), 0: go on, < 0: error.
static int long_front_checks(const LongPath &lp, const dd_params *p, const dd_device_batch *b, const dd_result *r, int w_begin, int w_end)
{
    int rc = check_params(p);
    if (rc) return rc;
    if (!b || !r || !r->ll || !r->status) return fail(DD_ERR_INVALID, "ll and status outputs are required");
    if (b->long_max_hap_len <= 0 || b->long_max_read_len <= 0 || b->n_haps <= 0 || b->n_reads <= 0 || w_end <= w_begin) return 1;
    if (!b->win_skip) return fail(DD_ERR_INVALID, std::string(lp.name) + ": win_skip must hold dd_screen_windows_ex's classes");
    return 0;
}

// The fields LongArgs and FLArgs name alike, from the batch; the model's own (read_flags, sym_lut, mate / library arrays, D, bMid) stay with the caller.
// ws_bytes: what the plan needs.  stats: the caller's device words, or NULL for the ones in the workspace header.
template <class Args>
static int long_fill_args(const LongPath &lp, Args &A, const dd_params *p, const dd_device_batch *b, const dd_result *r, void *workspace,
                          size_t workspace_bytes, uint64_t ws_bytes, int w_begin, int w_end, int read_begin, int read_end, unsigned long long *stats)
{
    if (!workspace || workspace_bytes < ws_bytes)
        return fail(DD_ERR_INVALID, std::string("workspace too small for the ") + lp.name + ": allocate " + lp.ws_fn + "() bytes");
    A.n_windows = b->n_windows; A.w_begin = w_begin; A.w_end = w_end; A.read_begin = read_begin; A.read_end = read_end;
    A.win_hap_off = b->win_hap_off; A.win_read_off = b->win_read_off; A.win_hap_start = b->win_hap_start;
    A.hap_seq_off = b->hap_seq_off; A.hap_seq = b->hap_seq; A.hap_var_off = b->hap_var_off; A.hap_var = b->hap_var; A.hap_var_flank = b->hap_var_flank;
    A.read_seq_off = b->read_seq_off; A.read_seq = b->read_seq; A.read_qidx = b->read_qidx; A.read_mqidx = b->read_mqidx;
    A.read_start = b->read_start;
    A.win_pair_off = b->win_pair_off; A.win_hpos_off = b->win_hpos_off; A.win_varcov_off = b->win_varcov_off;
    A.tables = b->tables; A.win_class = b->win_skip;
    A.out = *r;
    A.maxLengthDel = p->maxLengthDel; A.padCover = p->padCover; A.maxMismatch = p->maxMismatch;
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
// one long launch over the windows [w_begin, w_end) (their reads: [read_begin, read_end)); stats: device words the kernel counts into
static int launch_long_range(const dd_params *p, const dd_device_batch *b, const dd_result *r, void *workspace, size_t workspace_bytes,
                             void *stream, int w_begin, int w_end, int read_begin, int read_end, unsigned long long *stats)
{
    int rc = long_front_checks(g_long, p, b, r, w_begin, w_end);
    if (rc) return rc < 0 ? rc : DD_SUCCESS;
    ddl::LongArgs A;
    memset(&A, 0, sizeof(A));
    LongPlan lp;
    if ((rc = long_plan(b->n_windows, b->long_max_hap_len, b->long_max_read_len, b->n_qual, lp, A))) return rc;
    if ((rc = long_fill_args(g_long, A, p, b, r, workspace, workspace_bytes, lp.ws_bytes, w_begin, w_end, read_begin, read_end, stats))) return rc;
    A.read_flags = b->read_flags; A.sym_lut = b->sym_lut;
    if (p->mapUnmappedReads && (rc = fill_mate_args(A, b))) return rc;
    A.D = p->maxLengthDel + 1; A.bMid = p->bMid;
    A.max_read_len = b->long_max_read_len;
    A.off_lpoff = lp.off_lpoff; A.off_tiles = lp.off_tiles; A.tile_bytes = lp.tile_bytes; A.stash_off = lp.stash_off;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool onhap = r->onHap && r->offHapHMQ;
    HIP_TRY(ddl::launch_long(lp.K, A, lp.grid, lp.lds, onhap, st));
    const int64_t v[DD_LONG_LOG_FIELDS] = {(int64_t)lp.grid, -1, -1, (int64_t)lp.ws_bytes, lp.K, b->long_max_hap_len, b->long_max_read_len, (int64_t)lp.lds};
    long_log_push(g_long, v, A.stats, st);
    return DD_SUCCESS;
}

// ---------------- long windows of the --faster model (faster_long_kernel.hip) ----------------
// one launch over the windows [w_begin, w_end) (their reads: [read_begin, read_end)); stats: 4 device words the kernel counts into
static int launch_faster_long_range(const dd_params *p, const dd_device_batch *b, const dd_result *r, void *workspace, size_t workspace_bytes,
                                    void *stream, int w_begin, int w_end, int read_begin, int read_end, unsigned long long *stats)
{
    int rc = long_front_checks(g_flong, p, b, r, w_begin, w_end);
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
{   // the template instance this host thread launched last, as rocprofv3 prints it (inside "void ddk::...(ddk::KernelArgs)")
    const int K = g_last_launch[0], D = g_last_launch[1];
    if (K > 0 && D > 0) snprintf(g_kernel_name, sizeof(g_kernel_name), "dd_hmm_kernel<%d, %d, %s, %s, %d, %d>", K, D % 100, D >= 100 ? "true" : "false", g_last_fold ? "true" : "false", g_last_occ, g_last_G);
    else if (K > 0) snprintf(g_kernel_name, sizeof(g_kernel_name), "dd_faster_kernel");
    return g_kernel_name;
}

void dd_last_launch(int32_t out[8])
{   // K, D build, waves per workgroup, LDS bytes per workgroup, grid, read split, LDS per wave, shared LDS
    for (int i = 0; i < 8; i++) out[i] = g_last_launch[i];
}

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
    return launch_long_range(p, b, r, workspace, workspace_bytes, stream, 0, b->n_windows, 0, b->n_reads, nullptr);
}
int dd_long_launch_log(int64_t *out, int max_records) { return long_read_log(g_long, out, max_records); }   // see include/dindel_hmm.h

int dd_launch_device_faster_long(const dd_params *p, const dd_device_batch *b, const dd_result *r, void *workspace, size_t workspace_bytes, void *stream)
{
    g_flong.log.clear();
    if (!b) return fail(DD_ERR_INVALID, "null batch");
    return launch_faster_long_range(p, b, r, workspace, workspace_bytes, stream, 0, b->n_windows, 0, b->n_reads, nullptr);
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
