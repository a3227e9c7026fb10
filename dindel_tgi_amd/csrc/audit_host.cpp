// audit_host.cpp — the host arithmetic of an audit (include/dindel_hmm.h, "audit"): choosing the sample (dd_audit_select) and the CPU
// evaluation of the comparison (dd_audit_compare_host) from the header the kernel shares (audit_kernel.h).  No HIP runtime call, and it
// links without a kernel unit, like plan.cpp and batch_host.cpp (tests/audit_check.cpp builds the three under the sanitizers).  The device
// entries are audit_capi.cpp's.
#include "capi_internal.h"
#include "audit_kernel.h"

namespace ddh {
namespace {
bool window_eligible(const dd_batch *b, const uint8_t *win_class, int w)
{
    if (win_class && win_class[w] != DD_WIN_MAIN) return false;
    const int g0 = b->win_hap_off[w], g1 = b->win_hap_off[w + 1], q0 = b->win_read_off[w], q1 = b->win_read_off[w + 1];
    if (g1 <= g0 || q1 <= q0) return false;
    for (int g = g0; g < g1; g++) {
        const int len = b->hap_seq_off[g + 1] - b->hap_seq_off[g];
        if (len < 1 || len > DD_LONG_MAX_HAP_LEN) return false;
    }
    for (int q = q0; q < q1; q++) {
        const int len = b->read_seq_off[q + 1] - b->read_seq_off[q];
        if (len < 1 || len > DD_LONG_MAX_READ_LEN) return false;
    }
    return true;
}
} // namespace

// The geometry of the comparison from a host batch: the primary's offsets are worked out here (primary_off: 3 x (W + 1) entries).
int audit_geometry_host(const dd_batch *b, const dd_audit_view *view, std::vector<int64_t> &primary_off, au_geometry &G)
{
    const size_t W1 = (size_t)b->n_windows + 1;
    primary_off.assign(3 * W1, 0);
    const int rc = dd_batch_offsets(b, primary_off.data(), primary_off.data() + W1, primary_off.data() + 2 * W1);
    if (rc) return rc;
    G.n_windows = b->n_windows;
    G.win_hap_off = b->win_hap_off; G.win_read_off = b->win_read_off; G.read_seq_off = b->read_seq_off; G.hap_var_off = b->hap_var_off;
    G.win_pair_off = primary_off.data(); G.win_hpos_off = primary_off.data() + W1; G.win_varcov_off = primary_off.data() + 2 * W1;
    G.pair_off = view->pair_off; G.hpos_off = view->hpos_off; G.varcov_off = view->varcov_off;
    return DD_SUCCESS;
}

// What the entries that take a view check about it (the arrays' contents are the caller's: dd_audit_select wrote them).
int check_audit_view(const char *who, const dd_audit_view *v, int n_windows)
{
    if (!v) return fail(DD_ERR_INVALID, std::string(who) + ": null view");
    if (v->n_windows != n_windows) return fail(DD_ERR_INVALID, std::string(who) + ": the view was made for a batch of another number of windows");
    const dd_audit_sizes &s = v->sizes;
    if (s.n_windows < 0 || s.n_windows > n_windows || s.n_pairs < 0 || s.hpos_len < 0 || s.var_cov_len < 0 || s.max_hap_len < 0 || s.max_read_len < 0)
        return fail(DD_ERR_INVALID, std::string(who) + ": negative or impossible sizes in the view");
    if (s.n_pairs > 0 && (!v->audit_class || !v->pair_off || !v->hpos_off || !v->varcov_off))
        return fail(DD_ERR_INVALID, std::string(who) + ": null array in the view");
    return DD_SUCCESS;
}
} // namespace ddh

using namespace ddh;

extern "C" {

int dd_audit_select(const dd_params *p, const dd_batch *b, const uint8_t *win_class, uint64_t seed, int32_t n_want, uint8_t *audit_class,
                    int64_t *pair_off, int64_t *hpos_off, int64_t *varcov_off, dd_audit_sizes *sizes)
{
    int rc = check_params(p);
    if (rc) return rc;
    dd_sizes sz;
    if ((rc = dd_batch_sizes(b, &sz))) return rc;
    if (!audit_class || !pair_off || !hpos_off || !varcov_off || !sizes) return fail(DD_ERR_INVALID, "dd_audit_select: null output array");
    const int W = b->n_windows;
    std::vector<int> eligible;
    for (int w = 0; w < W; w++)
        if (window_eligible(b, win_class, w)) eligible.push_back(w);
    const int E = (int)eligible.size();
    const int want = n_want <= 0 ? 0 : n_want >= E ? E : n_want;
    std::vector<uint8_t> chosen((size_t)W, 0);
    AuditRng rng = {seed};
    int n_chosen = 0;
    if (want == E) {
        for (int w : eligible) chosen[(size_t)w] = 1;
        n_chosen = E;
    } else if (want > 0) {
        // step one: one window for every launch class that holds a haplotype of an eligible window, if the sample has room for all of them
        std::vector<uint8_t> ok((size_t)W, 0);
        for (int w : eligible) ok[(size_t)w] = 1;
        std::vector<uint8_t> skip((size_t)W, 0);           // the launch classes are built over the windows the main kernels compute
        bool any_skip = false;
        for (int w = 0; w < W; w++)
            if (win_class && win_class[w] != DD_WIN_MAIN) { skip[(size_t)w] = 1; any_skip = true; }
        std::vector<int32_t> list((size_t)sz.n_haps * DD_N_READ_CLASSES + 1), hap_window((size_t)sz.n_haps + 1);
        for (int w = 0; w < W; w++)
            for (int g = b->win_hap_off[w]; g < b->win_hap_off[w + 1]; g++) hap_window[(size_t)g] = w;
        dd_length_classes cls = {};
        if ((rc = build_launch_classes(b, any_skip ? skip.data() : nullptr, p, list.data(), &cls))) return rc;
        std::vector<std::vector<int>> class_windows;
        for (int i = 0; i < cls.n_launches; i++) {
            const dd_launch_class &L = cls.launch[i];
            std::vector<int> ws;
            for (int k = 0; k < L.list_len; k++) {
                const int w = hap_window[(size_t)list[(size_t)(L.list_off + k)]];
                if (ok[(size_t)w] && (ws.empty() || ws.back() != w)) ws.push_back(w);   // the list ascends: a window's haplotypes are adjacent
            }
            if (!ws.empty()) class_windows.push_back(ws);
        }
        if (want >= (int)class_windows.size())
            for (const std::vector<int> &ws : class_windows) {
                bool covered = false;
                for (int w : ws) covered = covered || chosen[(size_t)w];
                if (covered) continue;
                chosen[(size_t)ws[(size_t)rng.below(ws.size())]] = 1;
                n_chosen++;
            }
        // step two: the rest uniformly from the eligible windows not yet chosen (a partial Fisher-Yates shuffle)
        std::vector<int> rest;
        for (int w : eligible) if (!chosen[(size_t)w]) rest.push_back(w);
        for (size_t i = 0; n_chosen < want; i++, n_chosen++) {
            const size_t k = i + (size_t)rng.below(rest.size() - i);
            std::swap(rest[i], rest[k]);
            chosen[(size_t)rest[i]] = 1;
        }
    }
    // the shadow's layout: the batch's own (dd_batch_offsets), with every window that was not chosen at width 0
    memset(sizes, 0, sizeof(*sizes));
    int64_t np = 0, nh = 0, nc = 0;
    for (int w = 0; w < W; w++) {
        pair_off[w] = np; hpos_off[w] = nh; varcov_off[w] = nc;
        audit_class[w] = chosen[(size_t)w] ? DD_WIN_LONG : DD_WIN_UNSUPPORTED;
        if (!chosen[(size_t)w]) continue;
        const int g0 = b->win_hap_off[w], g1 = b->win_hap_off[w + 1], q0 = b->win_read_off[w], q1 = b->win_read_off[w + 1];
        const int64_t H = g1 - g0, R = q1 - q0, SL = b->read_seq_off[q1] - b->read_seq_off[q0];
        const int64_t nv = b->hap_var_off ? b->hap_var_off[g1] - b->hap_var_off[g0] : 0;
        np += H * R; nh += H * SL; nc += nv * R;
        for (int g = g0; g < g1; g++) sizes->max_hap_len = std::max(sizes->max_hap_len, b->hap_seq_off[g + 1] - b->hap_seq_off[g]);
        for (int q = q0; q < q1; q++) sizes->max_read_len = std::max(sizes->max_read_len, b->read_seq_off[q + 1] - b->read_seq_off[q]);
    }
    pair_off[W] = np; hpos_off[W] = nh; varcov_off[W] = nc;
    sizes->n_windows = n_chosen; sizes->n_pairs = np; sizes->hpos_len = nh; sizes->var_cov_len = nc;
    return E;
}

int dd_audit_compare_host(const dd_batch *b, const dd_result *primary, const dd_audit_view *view, const dd_result *shadow, void *report,
                          int64_t max_records)
{
    dd_sizes sz;
    int rc = dd_batch_sizes(b, &sz);
    if (rc) return rc;
    if (!primary || !shadow || !report) return fail(DD_ERR_INVALID, "dd_audit_compare_host: null primary, shadow or report");
    if (max_records < 0) return fail(DD_ERR_INVALID, "dd_audit_compare_host: negative max_records");
    if ((rc = check_audit_view("dd_audit_compare_host", view, b->n_windows))) return rc;
    dd_audit_report *rep = static_cast<dd_audit_report *>(report);
    dd_audit_record *records = reinterpret_cast<dd_audit_record *>(rep + 1);
    memset(report, 0, DD_AUDIT_REPORT_BYTES(max_records));
    if (view->sizes.n_pairs == 0) return DD_SUCCESS;
    if (!primary->ll || !primary->status || !shadow->ll || !shadow->status)
        return fail(DD_ERR_INVALID, "dd_audit_compare_host: ll and status are required on both sides");
    std::vector<int64_t> primary_off;
    au_geometry G;
    if ((rc = audit_geometry_host(b, view, primary_off, G))) return rc;
    const au_fields P = au_fields_of(primary), S = au_fields_of(shadow);
    const int has_flank = b->hap_var_flank != nullptr;
    auto differ = [&](const au_pair &a, int field, int64_t index, uint64_t x, uint64_t y) {
        rep->diff[field]++;
        if (rep->n_diff++ < max_records) records[rep->n_diff - 1] = {a.w, field, a.p_pair, index, x, y};
    };
    for (int64_t j = 0; j < view->sizes.n_pairs; j++) {
        const au_pair a = au_locate(&G, j);
        const int st_p = (int)au_load(P.f[DD_AUDIT_FIELD_status], a.p_pair, 4), st_s = (int)au_load(S.f[DD_AUDIT_FIELD_status], a.s_pair, 4);
        rep->n_pairs++;
        const uint32_t open = st_p == st_s ? au_compared(st_p, has_flank) : 1u << DD_AUDIT_FIELD_status;
        for (int f = 0; f < DD_AUDIT_N_FIELDS; f++) {
            if (!(open >> f & 1u) || !P.f[f] || !S.f[f]) continue;
            const int size = au_field_size(f);
            const bool per_pair = f < DD_AUDIT_N_PAIR_FIELDS;
            const int64_t p0 = per_pair ? a.p_pair : f == DD_AUDIT_FIELD_hpos ? a.p_hpos : a.p_cov;
            const int64_t s0 = per_pair ? a.s_pair : f == DD_AUDIT_FIELD_hpos ? a.s_hpos : a.s_cov;
            const int n = per_pair ? 1 : f == DD_AUDIT_FIELD_hpos ? a.L : a.nv;
            rep->compared[f] += n;
            for (int i = 0; i < n; i++) {
                const uint64_t x = au_load(P.f[f], p0 + i, size), y = au_load(S.f[f], s0 + i, size);
                if (x != y) differ(a, f, p0 + i, x, y);
            }
        }
    }
    return DD_SUCCESS;
}

} // extern "C"
