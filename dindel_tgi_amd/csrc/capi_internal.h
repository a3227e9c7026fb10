// capi_internal.h — what the host units of the C ABI (include/dindel_hmm.h) share: plan.cpp, batch_host.cpp (neither calls the HIP runtime
// nor needs a kernel unit to link), long_plan.cpp (the plans of the two long-window paths, with the layouts of their kernel units),
// launch.cpp, host_path.cpp, align_host.cpp (the haplotype alignment with the events and variants behind it), hapdist_host.cpp (the block
// table), pooled_em_capi.cpp (the pooled EM's device entries; pooled_em_host.cpp, its CPU evaluation, includes no HIP header and not this
// file), indel_keys_capi.cpp (the --faster model's indel-map key count: the launch and the CPU evaluation), audit_host.cpp (an audit's sample and
// the CPU evaluation of its comparison: no HIP runtime call either) and audit_capi.cpp (its device entries); each says in its first lines
// what it holds.  The last part of this file is what the host-pointer entries share: use_device, the
// arena slot, the one-shot arena of the three small entries and the record of a drawing kernel's last launch.  Host work is O(bases)
// bookkeeping only.  All likelihood arithmetic happens in the kernels; there is no CPU path for it in this library.
#ifndef DD_CAPI_INTERNAL_H
#define DD_CAPI_INTERNAL_H
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>
#include "hmm_kernel.h"
#include "long_kernel.h"
#include "faster_long_kernel.h"
#include "cigar_kernel.h"
#include "realign_kernel.h"
#include "draw_header.h"
#include "audit_kernel.h"

namespace ddh {
constexpr size_t kCuLdsBytes = 160u * 1024u;   // LDS of one CU (gfx950)
constexpr int kCUs = 256;                      // CUs of the chip

extern thread_local std::string g_err;         // dd_last_error(): per host thread (batch_host.cpp)
inline int fail(int code, const std::string &msg) { g_err = msg; return code; }

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return fail(DD_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));        \
    } while (0)

// options: the entry's option bits; DD_OPT_WIDE_DELETIONS lets maxLengthDel above 31 pass (an entry without options answers as ever)
inline int check_params(const dd_params *p, uint32_t options = 0)
{
    if (!p) return fail(DD_ERR_INVALID, "null params");
    if (p->forceReadOnHaplotype) return fail(DD_ERR_UNSUPPORTED, "forceReadOnHaplotype is not on the production path (DInDel.cpp:1446 only)");
    if ((options & DD_OPT_WIDE_DELETIONS) && p->maxLengthDel > DD_MAX_LENGTH_DEL) {
        if (p->maxLengthDel > DD_WIDE_MAX_LENGTH_DEL) return fail(DD_ERR_INVALID, "maxLengthDel above INT32_MAX - 2 (D = maxLengthDel + 1 is a 32-bit count)");
    } else if (p->maxLengthDel < 0 || p->maxLengthDel > DD_MAX_LENGTH_DEL) return fail(DD_ERR_UNSUPPORTED, "maxLengthDel outside [0,31]");
    if (!(p->pError > 0.0 && p->pError < 1.0)) return fail(DD_ERR_INVALID, "pError outside (0,1)");
    // each of these would put a NaN into dd_build_tables' output (log of a negative number, pow of a NaN), and the kernels' dmax() is
    // defined for non-NaN doubles only; the negated compares refuse a NaN field too
    if (!(p->pMut >= 0.0 && p->pMut <= 1.0)) return fail(DD_ERR_INVALID, "pMut outside [0,1]");
    if (!(p->pFirstgLO >= 0.0 && p->pFirstgLO <= 1.0)) return fail(DD_ERR_INVALID, "pFirstgLO outside [0,1]");
    if (!(p->mapQualThreshold >= 0.0)) return fail(DD_ERR_INVALID, "mapQualThreshold negative or NaN");
    if (!(p->capMapQualFast >= 0.0)) return fail(DD_ERR_INVALID, "capMapQualFast negative or NaN");
    if (p->checkBaseQualThreshold != p->checkBaseQualThreshold) return fail(DD_ERR_INVALID, "checkBaseQualThreshold is NaN");
    return DD_SUCCESS;
}

// which per-pair model an entry point runs
enum Model { MODEL_FBMAXERR = 0 /* ObservationModelFBMaxErr, computeLikelihoods */, MODEL_S = 1 /* ObservationModelS, computeLikelihoodsFaster */ };

// Every field of dd_result once, with the index space it lives in: PAIR one entry per pair, HPOS one per (pair, read base), VARCOV one per
// (pair, variant of its haplotype), READ one per read; and whether it may be written in place into the caller's page-locked memory (0: status
// and offHapHMQ stay in HBM, the onHap kernel reads them back).  The host-pointer path builds its list of output arrays from it (host_path.cpp,
// OutArray: placement in the arena, the in-place decision, downloads and the staged copy-back are each written once over that list, in
// this order: it is the order of the copies on a stream), and the multi-device front end its per-block pointer shift.
#define DD_RESULT_FIELDS(X)                                                                                                      \
    X(ll, PAIR, 1) X(llOn, PAIR, 1) X(llOff, PAIR, 1) X(mLogBQ, PAIR, 1) X(offHap, PAIR, 1) X(offHapHMQ, PAIR, 0) X(numIndels, PAIR, 1) \
    X(numMismatch, PAIR, 1) X(nBQT, PAIR, 1) X(nmmBQT, PAIR, 1) X(nMMLeft, PAIR, 1) X(nMMRight, PAIR, 1) X(firstBase, PAIR, 1)     \
    X(lastBase, PAIR, 1) X(status, PAIR, 0) X(hpos, HPOS, 1) X(var_covered, VARCOV, 1) X(var_fcov, VARCOV, 1) X(onHap, READ, 1)
enum ResultSpace { SPACE_PAIR, SPACE_HPOS, SPACE_VARCOV, SPACE_READ, SPACE_WINDOW /* one per window: dd_diploid_pair_result */ };
// Every field of dd_cigar_result (one entry per PAIR) and of dd_realign_result (one per READ), in the order the host-pointer path places and
// copies them, with the field's width: 1 = ops_cap elements per entry (ops), 0 = one.  None of them is written in place.
#define DD_CIGAR_FIELDS(X) X(n_ops, 0) X(ref_off, 0) X(status, 0) X(ops, 1)
#define DD_REALIGN_FIELDS(X) X(hap, 0) X(status, 0) X(n_ops, 0) X(ref_off, 0) X(ops, 1)
// Every field of dd_diploid_pair_result (one entry per WINDOW) with its width in elements.
#define DD_DIPPAIR_FIELDS(X) X(pair, 2) X(state, 1) X(best, 1) X(gap, 1) X(margin, 1)
#define DD_FIELD_SIZE(f, ...) + sizeof(S::f)
#define DD_LISTS_ALL_OF(T, FIELDS) static_assert([] { using S = T; return 0 FIELDS(DD_FIELD_SIZE); }() == sizeof(T), #FIELDS " must list every field of " #T)
DD_LISTS_ALL_OF(dd_result, DD_RESULT_FIELDS);
DD_LISTS_ALL_OF(dd_cigar_result, DD_CIGAR_FIELDS);
DD_LISTS_ALL_OF(dd_realign_result, DD_REALIGN_FIELDS);
DD_LISTS_ALL_OF(dd_diploid_pair_result, DD_DIPPAIR_FIELDS);
#undef DD_LISTS_ALL_OF
#undef DD_FIELD_SIZE

// ---- plan.cpp ----
// The A/B switches of plan.cpp, launch.cpp and build_launch_classes, read from the environment by read_switches() on every call (tests and
// tools flip them inside one process).  The arithmetic takes this struct and never calls getenv itself.  The switches of host_path.cpp and
// host/ stay where they are used; DD_LAUNCH_TIMING (launch.cpp) is read once per process.
struct Switches {
    bool no_half = false;               // DD_NO_HALF: whole-wavefront tilings only (test_launch_plan_rules, test_gpu_half_wave, tools/multi_round_sweep.py)
    int reg_waves = 0;                  // DD_REG_WAVES=1..16: waves per CU of a build compiled for another occupancy (tools/host_equivalence.py); 0: the shipped builds'
    int force_gbt = -1;                 // DD_FORCE_GBT=0/1: LDS / HBM-scratch back-pointers wherever that build fits (tools/plan_check.py, test_gpu_fuzz and others)
    int fast_groups = 0;                // DD_FAST_GROUPS=1/2: fewer pairs per wavefront of the --faster kernel (test_gpu_faster)
    int fast_waves = 0;                 // DD_FAST_WAVES=1..DD_WAVES: workgroup size of the --faster kernel (by hand only)
    int64_t fast_target_blocks = 1024;  // DD_FAST_TARGET_BLOCKS: workgroups wanted before the --faster kernel splits haplotypes (by hand only)
    bool always_ro = false;             // DD_ALWAYS_RO: KernelArgs::always_ro for the kernels (by hand only)
    int64_t target_blocks = 4096;       // DD_TARGET_BLOCKS: workgroups wanted before haplotypes are split (by hand only)
    bool split_no_rounds = false;       // DD_SPLIT_NO_ROUNDS: the read split without its round-fill term, the rule before round 3 (tools/README.md)
    bool uniform_split = false;         // DD_UNIFORM_SPLIT: no per-window split in ragged batches (test_gpu_ragged)
    int reads_per_wave = 0;             // DD_READS_PER_WAVE: cap on a wavefront's reads in ragged launches (test_gpu_ragged); 0: 12 or 24 by build
    int dynamic = -1;                   // DD_DYNAMIC=1 / any other value: the item counter wherever it can be used / never (test_gpu_ragged, test_gpu_persistent_rounds, tools/hostapi_time.py)
    bool no_fold = false;               // DD_NO_FOLD: no FOLD build, and no launches of their own for full-length haplotypes (test_gpu_fold_mirrored_ro, test_gpu_edge_cases)
    bool no_promote = false;            // DD_NO_PROMOTE: full-length haplotypes stay in their tiling's launch (test_full_length_haplotypes_leave_the_folded_launch)
    bool one_read_class = false;        // DD_LENGTH_CLASSES=k: launch classes by haplotype length only (test_gpu_ragged, tools/ragged_bench.py)
    int read_bound = -1;                // DD_READ_BOUND: the read length that cuts a tiling's reads up to 160 bp, in place of the plan's (tools/host_equivalence.py)
};
Switches read_switches();

struct HapClassDef { int bound, G, K; };     // haplotypes up to `bound` bp: G pairs per wavefront, K positions per lane
extern const HapClassDef kHapClasses[DD_N_HAP_CLASSES];
int hap_class_of(int hap_len);
bool pick_tiling(const Switches &sw, int max_hap_len, int Dt, int &G, int &K);
int pick_Dt(int D);

// the workspace starts with the item counter of the dynamic (ragged) launches; the back-pointer tiles follow
constexpr size_t DD_WS_HEADER = 256;

// Launch plan: LDS-resident back-pointers when that keeps the CU as full as the registers allow, otherwise
// the HBM-scratch build (GBT) with a persistent grid (one scratch tile per resident wave).
struct Plan {
    int K = 0, Dt = 0, waves = 0, waves_per_cu = 0;
    int G = 1;               // pairs per wavefront (2: the half-wave builds)
    bool gbt = false;
    bool two_waves = false;  // K = 3 / D = 6 scratch build: the variant compiled for 2 waves per SIMD (LDS keeps fewer than 12 waves on the CU anyway)
    size_t lds = 0, scratch_bytes = 0;
    unsigned grid_cap = 0;   // 0 = one workgroup per item
};
int lds_read_threshold(const Switches &sw, const dd_params *p, int max_hap_len, int n_qual);

// The scalars of one (haplotype-length class, read-length class) of a ragged batch: the launch is shaped for the class' own maxima
// instead of the batch-wide ones.
struct ClassDims {
    bool listed = false;                 // the class has a haplotype list: the launch covers [list_begin, list_end) of it
    int list_begin = 0, list_end = 0;
    int max_hap_len = 0, max_read_len = 0, min_read_len = 1;
    int max_window_reads = 0, avg_window_reads = 0;   // reads of the class per window of the list (0 = not known)
    int avg_read_len = 0;                             // mean length of the class' reads (0 = not known)
};
// What a main-model or --faster launch is shaped from: scalars only, no pointer into the batch and no device.
struct LaunchAsk {
    const dd_params *p = nullptr;
    int n_windows = 0, n_haps = 0, n_reads = 0, max_hap_len = 0, max_read_len = 0, n_qual = 0, max_window_reads = 0;   // of the batch
    bool has_class = false;
    ClassDims cls;
    int hap_begin = 0, hap_end = -1;     // the haplotypes the launch covers; hap_end < 0: the whole batch
    size_t workspace_bytes = 0;          // 0: no workspace
    bool overlapping_chunks = false;     // the caller alternates chunk launches between two streams (the host-pointer path)
};
// Every decision of a launch.  dd_last_launch, dd_kernel_name and a dd_launch_log record are made from it (shape_last_launch,
// shape_kernel_name, shape_log_record) and from nothing else.
struct LaunchShape {
    bool faster = false;                 // the --faster kernel: `groups` pairs per wavefront, no Plan
    Plan pl;
    int groups = 0;
    int waves = 0;                       // waves per workgroup and its LDS bytes, after the thin-window rule
    size_t lds = 0;
    uint32_t lds_wave_bytes = 0, lds_shared_bytes = 0;
    int64_t split = 0;                   // workgroups per haplotype of a window with the average number of reads
    int reads_per_wave = 0;              // > 0: ragged windows, the kernel derives each haplotype's workgroups from its window's reads
    int32_t item_begin = 0, n_items = 0;
    int64_t n_launch_items = 0, grid = 0;   // items of this launch; workgroups (fewer where the grid is persistent); grid <= 0: nothing to launch
    bool use_counter = false;            // the persistent grid draws its items from the counter at the start of the workspace
    bool fold = false;                   // the FOLD build (hmm_kernel.hip)
    int build = 0;                       // DD_BUILD_* bits
    int occ = 0;                         // the build variant compiled for that many waves per SIMD (0: the build's usual occupancy)
    int bt_rows = 0;                     // scratch builds: rows and bytes of a wavefront's back-pointer region, and where the regions start
    uint32_t bt_wave_bytes = 0;
    size_t scratch_off = 0;
    int n_haps = 0, max_hap = 0, min_read = 1, max_read = 0;   // what the launch covers (the class', or the batch's)
};
// Fill the LDS-layout fields of A and every field of s.  Errors, in this order: make_plan's, workspace too small, batch too large.
int shape_launch(const Switches &sw, const LaunchAsk &ask, LaunchShape &s, ddk::KernelArgs &A);
int shape_fast(const Switches &sw, const LaunchAsk &ask, LaunchShape &s, ddk::KernelArgs &A);
void shape_last_launch(const LaunchShape &s, int32_t out[8]);
void shape_kernel_name(const LaunchShape &s, char *name, size_t size);
void shape_log_record(const LaunchShape &s, int32_t v[DD_LAUNCH_LOG_FIELDS]);

// ---- long_plan.cpp ----
struct LongPlan { int K; size_t lds; unsigned grid; uint64_t off_lpoff, off_tiles, stash_off, tile_bytes, ws_bytes; };
int long_plan(int n_windows, int max_hap_len, int max_read_len, int n_qual, LongPlan &lp, ddl::LongArgs &A, bool wide = false);
// the wide build is asked for (DD_OPT_WIDE_DELETIONS) and needed (maxLengthDel > 31)
inline bool wide_on(const dd_params *p, uint32_t options) { return (options & DD_OPT_WIDE_DELETIONS) && p && p->maxLengthDel > DD_MAX_LENGTH_DEL; }
struct FLPlan { size_t lds; unsigned grid; uint64_t off_ioff, off_tiles, ws_bytes; };
int fl_plan(const dd_device_batch *b, FLPlan &fp, ddf::FLArgs &A);

// ---- batch_host.cpp ----
int assign_symbols(const dd_batch *b, uint8_t *out);
int screen_windows(const dd_batch *b, uint8_t *win_skip, int32_t max_len_out[2], const uint8_t *sym_lut, bool with_symbols);
int build_tables(const dd_params *p, const double *qual_table, int n_qual, const double *mapq_table, int n_mapq, double *out, uint32_t options);
int screen_windows_ex(const dd_params *p, const dd_batch *b, uint32_t options, uint8_t *win_class, int32_t max_len_out[4],
                      const uint8_t *sym_lut, bool with_symbols);
int build_launch_classes(const dd_batch *b, const uint8_t *win_skip, const dd_params *p, int32_t *list, dd_length_classes *out);

// ---- launch.cpp ----
// One launch class of a ragged batch: its scalars and the device copy of its haplotype list.
struct LenClass : ClassDims {
    const int32_t *hap_list = nullptr;   // device: haplotype indices of the class (sorted); nullptr = all haplotypes
    bool run_onhap = true;
};
// launch class L over its whole list; class_list: the device copy of the batch's class list
LenClass len_class_of(const dd_launch_class &L, const int32_t *class_list, bool run_onhap);
// Enqueue the path for haplotypes [hap_begin, hap_end) and reads [read_begin, read_end) of the batch (a
// contiguous block of windows); hap_end < 0 means the whole batch.
// overlapping_chunks: the caller alternates chunk launches between two streams (the host-pointer path)
int launch_range(Model model, const dd_params *p, const dd_device_batch *b, const dd_result *r, void *workspace, size_t workspace_bytes,
                 void *stream, int hap_begin, int hap_end, int read_begin, int read_end, bool overlapping_chunks, const LenClass *lc = nullptr,
                 uint32_t options = 0);
void launch_log_clear();
// the CIGAR launch (cigar_kernel.hip) over the pairs [pair_begin, pair_end) of the batch; pair_end < 0 = all of them (win_pair_off is a
// device array: a caller that wants a range knows its bounds)
int launch_cigars_range(const dd_device_batch *b, const int16_t *hpos_dev, const int32_t *status_dev, const int32_t *hap_ref_pos_dev,
                        const uint8_t *hap_aligned_dev, const dd_cigar_result *out_dev, int ops_cap, void *stream, int64_t pair_begin,
                        int64_t pair_end);
// the --faster model's indel-map key count (indel_keys_kernel.hip, enqueued by indel_keys_capi.cpp) over the pairs [pair_begin, pair_end)
// of the batch; pair_end < 0 = all of them
int launch_indel_keys_range(const dd_device_batch *b, const int16_t *hpos_dev, const int32_t *status_dev, int16_t *out_dev, void *stream,
                            int64_t pair_begin, int64_t pair_end);
// what one realign launch needs besides the batch (device pointers; dd_realign_device's arguments)
struct RealignInputs {
    int mode;
    const double *ll; const uint8_t *on_hap; const int32_t *win_hap_pair, *hap_n_indels;
    const int16_t *hpos; const int32_t *status, *hap_ref_pos; const uint8_t *hap_aligned;
};
// the realign launch (realign_kernel.hip) over the reads [read_begin, read_end) of the batch; read_end < 0 = all of them
int launch_realign_range(const dd_device_batch *b, const RealignInputs &in, const dd_realign_result *out_dev, int ops_cap, void *stream,
                         int read_begin, int read_end);

// ---- audit_host.cpp, audit_capi.cpp, faster_shadow_host.cpp, faster_shadow_capi.cpp ----
// splitmix64: the sample's only source of randomness, so that a choice is a function of the seed and the batch alone
struct AuditRng {
    uint64_t s;
    uint64_t next()
    {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    // uniform in [0, n), n >= 1: the draw is rejected while it lies in the short last stretch of the 64-bit range
    uint64_t below(uint64_t n)
    {
        const uint64_t limit = ~0ull - (~0ull % n + 1) % n;
        uint64_t v;
        do v = next(); while (v > limit);
        return v % n;
    }
};
// what the entries that take a dd_audit_view check about it; the comparison's geometry from a host batch (primary_off takes the primary's offsets)
int check_audit_view(const char *who, const dd_audit_view *v, int n_windows);
int audit_geometry_host(const dd_batch *b, const dd_audit_view *view, std::vector<int64_t> &primary_off, au_geometry &G);
// The audit of the chosen windows in [w_begin, w_end) (their reads: [read_begin, read_end)), enqueued on `stream` behind the likelihood
// launches of those windows: the long launch into `shadow`, then the comparison, which ADDS its counts to report_dev's header (the caller
// zeroes it) and draws its record slots from there.  j_begin, j_end: view->pair_off[w_begin], [w_end] (a device array: the caller knows
// them).  stats: two device words the long launch counts into, or NULL for the workspace header's.
int launch_audit_range(const dd_params *p, const dd_device_batch *b, const dd_result *primary, const dd_audit_view *view, const dd_result *shadow,
                       void *report_dev, int64_t max_records, void *workspace, size_t workspace_bytes, void *stream, int w_begin, int w_end,
                       int read_begin, int read_end, int64_t j_begin, int64_t j_end, unsigned long long *stats);

// The same for the --faster model (faster_shadow_capi.cpp): the shadow kernel over the sample's pairs [j_begin, j_end), then the comparison.
int launch_audit_faster_range(const dd_params *p, const dd_device_batch *b, const dd_result *primary, const dd_audit_view *view,
                              const dd_result *shadow, void *report_dev, int64_t max_records, void *workspace, void *stream, int64_t j_begin,
                              int64_t j_end);

static_assert(DD_LONG_LOG_FIELDS == DD_FASTER_LONG_LOG_FIELDS, "one record type serves both logs");
struct LongRec {
    int64_t v[DD_LONG_LOG_FIELDS];
    const unsigned long long *stats;     // device words the launch counts into
    hipStream_t stream;
};
// One long path: its name in the error texts, its stats words and the log fields they fill, and this thread's launch log.
struct LongPath {
    const char *name, *ws_fn;
    int n_stats, stat_field[4];          // stats word i -> log field stat_field[i] (-1: none); also the stride of compute_likelihoods' stats words per window block
    // (the last argument: the call's option bits, of which DD_OPT_WIDE_DELETIONS matters here)
    int (*launch_range)(const dd_params *, const dd_device_batch *, const dd_result *, void *, size_t, void *, int, int, int, int, unsigned long long *, uint32_t);
    size_t (*workspace_bytes)(const dd_params *, const dd_device_batch *);
    std::vector<LongRec> log;
};
extern thread_local LongPath g_long, g_flong;

// ---- what the host-pointer entries share (host_path.cpp and the one-shot entries of align_host.cpp, hapdist_host.cpp, pooled_em_capi.cpp) ----
// makes `device` current; no_device: the text when the machine has none
inline int use_device(int device, const char *no_device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(DD_ERR_NO_DEVICE, no_device);
    if (device < 0 || device >= ndev) return fail(DD_ERR_NO_DEVICE, "device ordinal out of range");
    HIP_TRY(hipSetDevice(device));
    return DD_SUCCESS;
}

// One array of a call in the device arena: its bytes, the pointer variable that takes its device address, and for an input the host array
// that is copied there.  A call lists every array it places before it touches the device, and the bytes it reserves are added up from those
// lists (HostCall::end_of_all, arena_layout): there is no size formula to keep in step with them.
struct ArenaSlot {
    size_t bytes;
    const unsigned char *src;                           // inputs: the host array (NULL: the array is only reserved)
    void *var; void (*set)(void *var, void *dev);       // the variable, written through its own type
    bool read_bases;                                    // read_seq / read_qidx, the two big inputs (HostCall::reserve_and_upload)
    void point_at(const void *dev) const { set(var, const_cast<void *>(dev)); }
};
template <class P> ArenaSlot arena_slot(P *var, size_t bytes, const void *src = nullptr, bool read_bases = false)
{
    return {bytes, static_cast<const unsigned char *>(src), var, [](void *v, void *dev) { *static_cast<P *>(v) = static_cast<P>(dev); }, read_bases};
}

// The one-shot arena of the small entries (one allocation per call, freed with it).  Its layout, without a HIP call: every slot starts at a
// multiple of 256 bytes, and an array of 0 bytes takes 1, so that it has an address of its own.  off[i]: where slot i starts; returns the total.
inline size_t arena_layout(const std::vector<ArenaSlot> &slots, std::vector<size_t> &off)
{
    size_t at = 0;
    off.clear();
    for (const ArenaSlot &s : slots) {
        off.push_back(at);
        at = (at + std::max<size_t>(s.bytes, 1) + 255u) & ~size_t(255u);
    }
    return at;
}
inline void arena_point(const std::vector<ArenaSlot> &slots, const std::vector<size_t> &off, unsigned char *base)
{
    for (size_t i = 0; i < slots.size(); i++) slots[i].point_at(base + off[i]);
}
struct OneShotArena {
    unsigned char *base = nullptr;
    size_t bytes = 0;
    OneShotArena() = default;
    OneShotArena(const OneShotArena &) = delete;
    ~OneShotArena() { if (base) (void)hipFree(base); }
    bool holds(const void *p) const { return base && p >= base && p < base + bytes; }
    // allocate what the slots add up to, point every slot's variable at its piece and upload the slots that have a source
    int place(const std::vector<ArenaSlot> &slots)
    {
        std::vector<size_t> off;
        bytes = arena_layout(slots, off);
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&base), bytes));
        arena_point(slots, off, base);
        for (size_t i = 0; i < slots.size(); i++)
            if (slots[i].src && slots[i].bytes) HIP_TRY(hipMemcpy(base + off[i], slots[i].src, slots[i].bytes, hipMemcpyHostToDevice));
        return DD_SUCCESS;
    }
};
// the copy back: each array the caller has room for (0 bytes: none)
struct Download { void *dst; const void *dev; size_t bytes; };
inline int download(std::initializer_list<Download> list)
{
    for (const Download &d : list)
        if (d.bytes) HIP_TRY(hipMemcpy(d.dst, d.dev, d.bytes, hipMemcpyDeviceToHost));
    return DD_SUCCESS;
}

// This thread's last launch of a kernel whose wavefronts draw their items from a counter (draw_header.h): n int64 fields, of which the last
// two come from the device (most draws of one wavefront, guard trips).  They are read on demand from the launch's three header words, or
// cached by a host entry, whose workspace does not outlive the call.
struct LaunchRecord {
    int64_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int n;
    const unsigned int *hdr = nullptr;   // device: the header the launch counts into (NULL: no launch yet, or its workspace is gone)
    int base = 0;                        // the launch's first word in it
    hipStream_t stream = nullptr;
    bool have_stats = true;
    explicit LaunchRecord(int n_fields) : n(n_fields) {}
    // in front of a launch: its host-side fields (n - 2 of them), and where and behind what its device words will be
    void note(std::initializer_list<int64_t> host_fields, const void *header, int base_word, void *st)
    {
        std::copy(host_fields.begin(), host_fields.end(), v);
        v[n - 2] = v[n - 1] = -1;
        hdr = static_cast<const unsigned int *>(header); base = base_word; stream = static_cast<hipStream_t>(st); have_stats = false;
    }
    int read_stats()
    {
        if (have_stats || !hdr) return DD_SUCCESS;
        uint32_t w[DD_DRAW_WORDS];
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipMemcpy(w, hdr + base, sizeof(w), hipMemcpyDeviceToHost));
        v[n - 2] = w[DD_DRAW_MAX_DRAWS]; v[n - 1] = w[DD_DRAW_TRIPS];
        have_stats = true;
        return DD_SUCCESS;
    }
    void forget() { hdr = nullptr; }     // the workspace is gone: what has been read stays
    void copy_out(int64_t *out)          // a dd_*_last_launch
    {
        (void)read_stats();              // a failure leaves -1 in the two device fields
        if (out) memcpy(out, v, (size_t)n * sizeof(*v));
    }
};
// The records of the launches a host entry runs in its arena.  read_stats() caches their device words (the success path reports a failure
// of that); on every way out of the entry the destructor does the same and then forgets the workspace.  It is made from the arena, so it
// is declared behind it and gone before it: no record outlives the memory it points into.  A record of an earlier launch elsewhere is left alone.
struct ArenaRecords {
    const OneShotArena &arena;
    std::vector<LaunchRecord *> recs;
    ArenaRecords(const OneShotArena &a, std::initializer_list<LaunchRecord *> r) : arena(a), recs(r) {}
    int read_stats()
    {
        for (LaunchRecord *r : recs)
            if (arena.holds(r->hdr)) { const int rc = r->read_stats(); if (rc) return rc; }
        return DD_SUCCESS;
    }
    ~ArenaRecords()
    {
        for (LaunchRecord *r : recs)
            if (arena.holds(r->hdr)) {
                const std::string err = g_err;           // the entry's own error text stands
                if (r->read_stats()) g_err = err;
                r->forget();
            }
    }
};
} // namespace ddh
#endif
