// audit_capi.cpp — the device entries of an audit (include/dindel_hmm.h, "audit"): the workspace size, the launch over the whole sample
// (dd_audit_device) or over the chosen windows of a window block (launch_audit_range: the host-pointer entry, dd_compute_likelihoods_audit,
// is a request of host_path.cpp's call), and the record of the audit's long launch.  The long-window kernel is used as it stands, through
// the long path's own launcher (g_long.launch_range), on a copy of the batch whose window classes, output offsets and long maxima are the
// sample's; the comparison is audit_kernel.hip.  The sample and the CPU evaluation are audit_host.cpp's.
#include "capi_internal.h"

namespace ddh {
namespace {
struct AuditRec {
    LongRec rec = {{0, 0, 0, 0, 0, 0, 0, 0}, nullptr, nullptr};
    int64_t compare_grid = 0;
};
thread_local AuditRec g_audit_rec;

// the long plan of a sample
int audit_plan(const dd_audit_view *v, LongPlan &lp)
{
    ddl::LongArgs A;
    memset(&A, 0, sizeof(A));
    return long_plan(v->n_windows, v->sizes.max_hap_len, v->sizes.max_read_len, v->n_qual, lp, A);
}
} // namespace

int launch_audit_range(const dd_params *p, const dd_device_batch *b, const dd_result *primary, const dd_audit_view *view, const dd_result *shadow,
                       void *report_dev, int64_t max_records, void *workspace, size_t workspace_bytes, void *stream, int w_begin, int w_end,
                       int read_begin, int read_end, int64_t j_begin, int64_t j_end, unsigned long long *stats)
{
    if (j_end <= j_begin) return DD_SUCCESS;
    // the batch as the long launch shall see it: the chosen windows are its long windows, and they lie in the shadow where the sample puts them
    dd_device_batch lb = *b;
    lb.win_skip = view->audit_class;
    lb.win_pair_off = view->pair_off; lb.win_hpos_off = view->hpos_off; lb.win_varcov_off = view->varcov_off;
    lb.long_max_hap_len = view->sizes.max_hap_len; lb.long_max_read_len = view->sizes.max_read_len;
    lb.classes = nullptr; lb.hap_class_list = nullptr;
    dd_result sh = *shadow;
    sh.onHap = nullptr;                                    // derived per read of the batch: the shadow has none
    // the launcher appends to the long path's log, which belongs to the likelihood call: the record moves to the audit's own
    std::vector<LongRec> kept;
    kept.swap(g_long.log);
    const int rc = g_long.launch_range(p, &lb, &sh, workspace, workspace_bytes, stream, w_begin, w_end, read_begin, read_end, stats, 0);
    kept.swap(g_long.log);
    if (rc) return rc;
    if (!kept.empty()) g_audit_rec.rec = kept.back();

    dda::AuditArgs A;
    memset(&A, 0, sizeof(A));
    A.G.n_windows = b->n_windows;
    A.G.win_hap_off = b->win_hap_off; A.G.win_read_off = b->win_read_off; A.G.read_seq_off = b->read_seq_off; A.G.hap_var_off = b->hap_var_off;
    A.G.win_pair_off = b->win_pair_off; A.G.win_hpos_off = b->win_hpos_off; A.G.win_varcov_off = b->win_varcov_off;
    A.G.pair_off = view->pair_off; A.G.hpos_off = view->hpos_off; A.G.varcov_off = view->varcov_off;
    A.primary = au_fields_of(primary); A.shadow = au_fields_of(&sh);
    A.has_flank = b->hap_var_flank != nullptr;
    A.j_begin = j_begin; A.j_end = j_end;
    A.report = static_cast<dd_audit_report *>(report_dev);
    A.records = reinterpret_cast<dd_audit_record *>(A.report + 1);
    A.max_records = max_records;
    HIP_TRY(dda::launch_audit_compare(A, static_cast<hipStream_t>(stream)));
    g_audit_rec.compare_grid = dda::audit_grid(j_end - j_begin);
    return DD_SUCCESS;
}
} // namespace ddh

using namespace ddh;

extern "C" {

size_t dd_audit_workspace_bytes(const dd_params *p, const dd_audit_view *view)
{
    (void)p;
    if (!view || view->sizes.n_pairs <= 0 || view->sizes.max_hap_len <= 0 || view->sizes.max_read_len <= 0) return 0;
    LongPlan lp;
    if (audit_plan(view, lp)) return 0;
    return (size_t)lp.ws_bytes;
}

int dd_audit_device(const dd_params *p, const dd_device_batch *b, const dd_result *primary, const dd_audit_view *view, const dd_result *shadow,
                    void *report_dev, int64_t max_records, void *workspace, size_t workspace_bytes, void *stream)
{
    g_audit_rec = AuditRec();
    int rc = check_params(p);
    if (rc) return rc;
    if (!b || !primary || !shadow || !report_dev) return fail(DD_ERR_INVALID, "dd_audit_device: null batch, primary, shadow or report");
    if (max_records < 0) return fail(DD_ERR_INVALID, "dd_audit_device: negative max_records");
    if (reinterpret_cast<uintptr_t>(report_dev) % 8) return fail(DD_ERR_INVALID, "dd_audit_device: the report must be 8-byte aligned");
    if (b->n_windows < 0 || b->n_haps < 0 || b->n_reads < 0) return fail(DD_ERR_INVALID, "dd_audit_device: negative count");
    if ((rc = check_audit_view("dd_audit_device", view, b->n_windows))) return rc;
    if (view->n_qual != b->n_qual) return fail(DD_ERR_INVALID, "dd_audit_device: the view was made for a batch with another quality table");
    const bool work = view->sizes.n_pairs > 0 && b->n_haps > 0 && b->n_reads > 0;
    if (work) {
        if (!primary->ll || !primary->status || !shadow->ll || !shadow->status)
            return fail(DD_ERR_INVALID, "dd_audit_device: ll and status are required on both sides");
        if (!b->win_hap_off || !b->win_read_off || !b->read_seq_off || !b->win_pair_off || !b->win_hpos_off || !b->win_varcov_off)
            return fail(DD_ERR_INVALID, "dd_audit_device: null offset array");
        LongPlan lp;
        if ((rc = audit_plan(view, lp))) return rc;
        if (!workspace || workspace_bytes < lp.ws_bytes)
            return fail(DD_ERR_INVALID, "workspace too small for the audit: allocate dd_audit_workspace_bytes() bytes");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return fail(DD_ERR_NO_DEVICE, "no HIP device: the audit's device entry has no CPU fallback (dd_audit_compare_host compares host arrays)");
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(report_dev, 0, DD_AUDIT_REPORT_BYTES(max_records), st));    // the records too: unused slots read zero
    if (!work) return DD_SUCCESS;
    return launch_audit_range(p, b, primary, view, shadow, report_dev, max_records, workspace, workspace_bytes, stream, 0, b->n_windows, 0,
                              b->n_reads, 0, view->sizes.n_pairs, nullptr);
}

void dd_audit_last_launch(int64_t out[DD_AUDIT_LOG_FIELDS])
{
    AuditRec &a = g_audit_rec;
    LongRec &r = a.rec;
    if (r.stats && r.v[1] < 0) {
        unsigned long long st[2] = {0, 0};
        if (hipStreamSynchronize(r.stream) == hipSuccess && hipMemcpy(st, r.stats, sizeof(st), hipMemcpyDeviceToHost) == hipSuccess) {
            r.v[1] = (int64_t)st[0]; r.v[2] = (int64_t)st[1];
        } else {
            (void)hipGetLastError();
        }
    }
    if (!out) return;
    for (int i = 0; i < 7; i++) out[i] = r.v[i];
    out[7] = a.compare_grid;
}

} // extern "C"
