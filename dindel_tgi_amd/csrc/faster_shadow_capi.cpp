// faster_shadow_capi.cpp — the device entries of an audit of the --faster model (include/dindel_hmm.h, "audit of the --faster model"): the
// workspace size, the launch over the whole sample (dd_audit_device_faster: the shadow kernel, then the comparison under this model's
// rule; both faster_shadow_kernel.hip), the same over the chosen windows of a window block (launch_audit_faster_range: the host-pointer entry,
// dd_compute_likelihoods_faster_audit, is a request of host_path.cpp's call) and the record of that launch.  The sample, the CPU shadow and the CPU comparison are
// faster_shadow_host.cpp's.
#include "capi_internal.h"
#include "faster_shadow.h"

namespace ddh {
namespace {
struct ShadowRec { int64_t v[DD_AUDIT_LOG_FIELDS] = {0, 0, 0, 0, 0, 0, 0, 0}; };
thread_local ShadowRec g_shadow_rec;

bool shapes_ok(const dd_audit_sizes &s)
{
    return s.max_hap_len > 0 && s.max_read_len > 0 && s.max_hap_len <= DD_LONG_MAX_HAP_LEN && s.max_read_len <= DD_LONG_MAX_READ_LEN;
}
size_t shadow_ws_bytes(const dd_audit_sizes &s)
{
    if (dfs::area_in_lds(s.max_hap_len, s.max_read_len)) return 0;
    return (size_t)dfs::shadow_grid(s.n_pairs, s.max_hap_len, s.max_read_len) * DD_FS_WAVES * dfs::area_bytes(s.max_hap_len, s.max_read_len);
}
} // namespace

// The audit of the sample's pairs [j_begin, j_end) (the chosen windows of a window block), enqueued on `stream` behind the --faster launches
// of those windows: the shadow kernel into `shadow`, then the comparison, which ADDS its counts to report_dev's header (the caller zeroes
// it) and draws its record slots from there.  workspace: dd_audit_workspace_bytes_faster(view) bytes, or anything when that is 0.
int launch_audit_faster_range(const dd_params *p, const dd_device_batch *b, const dd_result *primary, const dd_audit_view *view,
                              const dd_result *shadow, void *report_dev, int64_t max_records, void *workspace, void *stream, int64_t j_begin,
                              int64_t j_end)
{
    if (j_end <= j_begin) return DD_SUCCESS;
    const dd_audit_sizes &s = view->sizes;
    const size_t ws_need = shadow_ws_bytes(s);
    hipStream_t st = static_cast<hipStream_t>(stream);
    dfs::ShadowArgs A;
    memset(&A, 0, sizeof(A));
    A.G.n_windows = b->n_windows;
    A.G.win_hap_off = b->win_hap_off; A.G.win_read_off = b->win_read_off; A.G.read_seq_off = b->read_seq_off; A.G.hap_var_off = b->hap_var_off;
    A.G.win_pair_off = b->win_pair_off; A.G.win_hpos_off = b->win_hpos_off; A.G.win_varcov_off = b->win_varcov_off;
    A.G.pair_off = view->pair_off; A.G.hpos_off = view->hpos_off; A.G.varcov_off = view->varcov_off;
    A.win_hap_start = b->win_hap_start; A.hap_seq_off = b->hap_seq_off; A.hap_seq = b->hap_seq;
    A.hap_var = b->hap_var; A.hap_var_flank = b->hap_var_flank;
    A.read_seq = b->read_seq; A.read_qidx = b->read_qidx; A.read_mqidx = b->read_mqidx; A.read_start = b->read_start;
    A.tables = b->tables;
    A.out = *shadow;
    A.out.onHap = nullptr;                                  // derived per read of the batch: the shadow has none
    A.maxLengthDel = p->maxLengthDel; A.padCover = p->padCover; A.maxMismatch = p->maxMismatch;
    A.max_hap_len = s.max_hap_len; A.max_read_len = s.max_read_len;
    A.j_begin = j_begin; A.j_end = j_end;
    A.ws = ws_need ? static_cast<unsigned char *>(workspace) : nullptr;
    HIP_TRY(dfs::launch_shadow(A, st));

    dda::AuditArgs C;
    memset(&C, 0, sizeof(C));
    C.G = A.G;
    C.primary = au_fields_of(primary); C.shadow = au_fields_of(&A.out);
    C.has_flank = b->hap_var_flank != nullptr;
    C.j_begin = j_begin; C.j_end = j_end;
    C.report = static_cast<dd_audit_report *>(report_dev);
    C.records = reinterpret_cast<dd_audit_record *>(C.report + 1);
    C.max_records = max_records;
    HIP_TRY(dfs::launch_compare_faster(C, st));

    const int64_t n = j_end - j_begin;
    int64_t *v = g_shadow_rec.v;
    v[0] = dfs::shadow_grid(n, s.max_hap_len, s.max_read_len); v[1] = n; v[2] = ws_need ? 0 : 1; v[3] = (int64_t)ws_need;
    v[4] = (int64_t)dfs::shadow_lds_bytes(s.max_hap_len, s.max_read_len); v[5] = s.max_hap_len; v[6] = s.max_read_len;
    v[7] = std::min<int64_t>((n + DD_FS_WAVES - 1) / DD_FS_WAVES, DD_FS_MAX_BLOCKS);
    return DD_SUCCESS;
}
} // namespace ddh

using namespace ddh;

extern "C" {

size_t dd_audit_workspace_bytes_faster(const dd_params *p, const dd_audit_view *view)
{
    (void)p;
    if (!view || view->sizes.n_pairs <= 0 || !shapes_ok(view->sizes)) return 0;
    return shadow_ws_bytes(view->sizes);
}

int dd_audit_device_faster(const dd_params *p, const dd_device_batch *b, const dd_result *primary, const dd_audit_view *view,
                           const dd_result *shadow, void *report_dev, int64_t max_records, void *workspace, size_t workspace_bytes, void *stream)
{
    g_shadow_rec = ShadowRec();
    int rc = check_params(p);
    if (rc) return rc;
    if (!b || !primary || !shadow || !report_dev) return fail(DD_ERR_INVALID, "dd_audit_device_faster: null batch, primary, shadow or report");
    if (max_records < 0) return fail(DD_ERR_INVALID, "dd_audit_device_faster: negative max_records");
    if (reinterpret_cast<uintptr_t>(report_dev) % 8) return fail(DD_ERR_INVALID, "dd_audit_device_faster: the report must be 8-byte aligned");
    if (b->n_windows < 0 || b->n_haps < 0 || b->n_reads < 0) return fail(DD_ERR_INVALID, "dd_audit_device_faster: negative count");
    if ((rc = check_audit_view("dd_audit_device_faster", view, b->n_windows))) return rc;
    if (view->n_qual != b->n_qual) return fail(DD_ERR_INVALID, "dd_audit_device_faster: the view was made for a batch with another quality table");
    const dd_audit_sizes &s = view->sizes;
    const bool work = s.n_pairs > 0 && b->n_haps > 0 && b->n_reads > 0;
    size_t ws_need = 0;
    if (work) {
        if (!primary->ll || !primary->status || !shadow->ll || !shadow->status)
            return fail(DD_ERR_INVALID, "dd_audit_device_faster: ll and status are required on both sides");
        if (!b->win_hap_off || !b->win_read_off || !b->read_seq_off || !b->win_pair_off || !b->win_hpos_off || !b->win_varcov_off)
            return fail(DD_ERR_INVALID, "dd_audit_device_faster: null offset array");
        if (!b->win_hap_start || !b->hap_seq_off || !b->hap_seq || !b->read_seq || !b->read_qidx || !b->read_mqidx || !b->read_start || !b->tables)
            return fail(DD_ERR_INVALID, "dd_audit_device_faster: null input array (the shadow reads the batch the launch read)");
        if (s.var_cov_len > 0 && (!b->hap_var_off || !b->hap_var))
            return fail(DD_ERR_INVALID, "dd_audit_device_faster: the sample has variants, the batch has no hap_var_off / hap_var");
        if (!shapes_ok(s)) return fail(DD_ERR_INVALID, "dd_audit_device_faster: the sample holds a shape beyond the long limits");
        ws_need = shadow_ws_bytes(s);
        if (ws_need && (!workspace || workspace_bytes < ws_need))
            return fail(DD_ERR_INVALID, "workspace too small for the audit: allocate dd_audit_workspace_bytes_faster() bytes");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return fail(DD_ERR_NO_DEVICE, "no HIP device: the audit's device entry has no CPU fallback (dd_audit_shadow_faster_host and "
                                      "dd_audit_compare_host_faster work on host arrays)");
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(report_dev, 0, DD_AUDIT_REPORT_BYTES(max_records), st));    // the records too: unused slots read zero
    if (!work) return DD_SUCCESS;

    return launch_audit_faster_range(p, b, primary, view, shadow, report_dev, max_records, workspace, stream, 0, s.n_pairs);
}

void dd_audit_last_launch_faster(int64_t out[DD_AUDIT_LOG_FIELDS])
{
    if (out) memcpy(out, g_shadow_rec.v, sizeof(g_shadow_rec.v));
}

} // extern "C"
