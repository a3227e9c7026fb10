// faster_shadow_host.cpp — the host arithmetic of an audit of the --faster model (include/dindel_hmm.h, "audit of the --faster model"):
// choosing the sample (dd_audit_select_faster), the shadow on the CPU (dd_audit_shadow_faster_host: faster_shadow.h's functions looped
// over the sample's pairs and their destination states, as the shadow kernel runs them over lanes) and the CPU evaluation of the
// comparison under this model's rule (dd_audit_compare_host_faster).  No HIP runtime call, and it links without a kernel unit, like
// audit_host.cpp (tests/audit_faster_check.cpp builds it with audit_host.cpp, batch_host.cpp and plan.cpp under the sanitizers).  The
// device entries are faster_shadow_capi.cpp's.
#include "capi_internal.h"
#include "faster_shadow.h"

namespace ddh {
namespace {
// the class a --faster launch gives window w: win_class' byte, or by shape when there is none; -1: nothing can compute it
int faster_class(const dd_batch *b, const uint8_t *win_class, int w)
{
    const int g0 = b->win_hap_off[w], g1 = b->win_hap_off[w + 1], q0 = b->win_read_off[w], q1 = b->win_read_off[w + 1];
    if (g1 <= g0 || q1 <= q0) return -1;
    bool is_long = false;
    for (int g = g0; g < g1; g++) {
        const int len = b->hap_seq_off[g + 1] - b->hap_seq_off[g];
        if (len < 1 || len > DD_LONG_MAX_HAP_LEN) return -1;
        is_long = is_long || len > DD_MAX_HAP_LEN;
    }
    for (int q = q0; q < q1; q++) {
        const int len = b->read_seq_off[q + 1] - b->read_seq_off[q];
        if (len < 1 || len > DD_LONG_MAX_READ_LEN) return -1;
        is_long = is_long || len > DD_MAX_READ_LEN;
    }
    if (win_class) return win_class[w];
    return is_long ? DD_WIN_LONG : DD_WIN_MAIN;
}

template <class T> void put(T *field, int64_t at, T v) { if (field) field[at] = v; }
} // namespace
} // namespace ddh

using namespace ddh;

extern "C" {

int dd_audit_select_faster(const dd_params *p, const dd_batch *b, const uint8_t *win_class, uint32_t options, uint64_t seed, int32_t n_want,
                           uint8_t *audit_class, int64_t *pair_off, int64_t *hpos_off, int64_t *varcov_off, dd_audit_sizes *sizes)
{
    int rc = check_params(p);
    if (rc) return rc;
    dd_sizes sz;
    if ((rc = dd_batch_sizes(b, &sz))) return rc;
    if (options & ~DD_OPT_LONG_WINDOWS_FASTER) return fail(DD_ERR_INVALID, "dd_audit_select_faster: unknown option (0 or DD_OPT_LONG_WINDOWS_FASTER)");
    if (!audit_class || !pair_off || !hpos_off || !varcov_off || !sizes) return fail(DD_ERR_INVALID, "dd_audit_select_faster: null output array");
    const int W = b->n_windows;
    const bool with_long = (options & DD_OPT_LONG_WINDOWS_FASTER) != 0;
    std::vector<int> eligible, long_ones;
    int w_hap = -1, w_read = -1, best_hap = 0, best_read = 0;       // the windows holding the longest ordinary haplotype / read
    for (int w = 0; w < W; w++) {
        const int c = faster_class(b, win_class, w);
        if (c == DD_WIN_MAIN) {
            eligible.push_back(w);
            for (int g = b->win_hap_off[w]; g < b->win_hap_off[w + 1]; g++) {
                const int len = b->hap_seq_off[g + 1] - b->hap_seq_off[g];
                if (len <= DD_MAX_HAP_LEN && len > best_hap) { best_hap = len; w_hap = w; }
            }
            for (int q = b->win_read_off[w]; q < b->win_read_off[w + 1]; q++) {
                const int len = b->read_seq_off[q + 1] - b->read_seq_off[q];
                if (len <= DD_MAX_READ_LEN && len > best_read) { best_read = len; w_read = w; }
            }
        } else if (c == DD_WIN_LONG && with_long) {
            eligible.push_back(w);
            long_ones.push_back(w);
        }
    }
    const int E = (int)eligible.size();
    const int want = n_want <= 0 ? 0 : n_want >= E ? E : n_want;
    std::vector<uint8_t> chosen((size_t)W, 0);
    AuditRng rng = {seed};
    int n_chosen = 0;
    if (want == E) {
        for (int w : eligible) chosen[(size_t)w] = 1;
        n_chosen = E;
    } else if (want > 0) {
        // step one: the two shapes that size the --faster launch's LDS and one long window, if the sample has room for all of them
        const int n_first = (w_hap >= 0) + (w_read >= 0 && w_read != w_hap) + (long_ones.empty() ? 0 : 1);
        if (want >= n_first) {
            for (int w : {w_hap, w_read})
                if (w >= 0 && !chosen[(size_t)w]) { chosen[(size_t)w] = 1; n_chosen++; }
            if (!long_ones.empty()) { chosen[(size_t)long_ones[(size_t)rng.below(long_ones.size())]] = 1; n_chosen++; }
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

int dd_audit_shadow_faster_host(const dd_params *p, const dd_batch *b, const dd_audit_view *view, const dd_result *shadow)
{
    int rc = check_params(p);
    if (rc) return rc;
    dd_sizes sz;
    if ((rc = dd_batch_sizes(b, &sz))) return rc;
    if (!shadow) return fail(DD_ERR_INVALID, "dd_audit_shadow_faster_host: null shadow");
    if ((rc = check_audit_view("dd_audit_shadow_faster_host", view, b->n_windows))) return rc;
    if (view->sizes.n_pairs == 0) return DD_SUCCESS;
    if (!shadow->ll || !shadow->status) return fail(DD_ERR_INVALID, "dd_audit_shadow_faster_host: ll and status are required in the shadow");
    if (view->sizes.max_hap_len > DD_LONG_MAX_HAP_LEN || view->sizes.max_read_len > DD_LONG_MAX_READ_LEN)
        return fail(DD_ERR_INVALID, "dd_audit_shadow_faster_host: the sample holds a shape beyond the long limits");
    std::vector<double> T(DD_TABLE_DOUBLES, 0.0);
    if ((rc = dd_build_tables(p, b->qual_table, b->n_qual, b->mapq_table, b->n_mapq, T.data())) < 0) return rc;
    std::vector<int64_t> primary_off;
    au_geometry G;
    if ((rc = audit_geometry_host(b, view, primary_off, G))) return rc;

    const size_t maxL = (size_t)view->sizes.max_read_len, maxH = (size_t)view->sizes.max_hap_len;
    std::vector<int32_t> hist(maxL + maxH + 1);
    std::vector<uint8_t> rk(maxL + 1), bt((maxL + 1) * FS_MAX_STATES), path(maxL + 1);
    std::vector<int16_t> ms(maxL + 1);
    uint32_t bits[FS_COV_WORDS];
    int32_t rel[FS_MAX_DIAGONALS + 1];
    double row[2][FS_MAX_STATES] = {}, left[FS_MAX_STATES] = {}, right[FS_MAX_STATES] = {};   // (a side without bases is passed on, never added)
    const dd_result &o = *shadow;

    for (int64_t j = 0; j < view->sizes.n_pairs; j++) {
        const fs_where x = fs_locate(&G, j);
        const au_pair &a = x.a;
        const int hs = b->hap_seq_off[x.g], hlen = b->hap_seq_off[x.g + 1] - hs, so = b->read_seq_off[x.q], L = a.L;
        const int v0 = a.nv > 0 ? b->hap_var_off[x.g] : 0;
        const int status = fs_status(p->maxLengthDel, hlen, L);
        // the fields this model leaves at MLAlignment's defaults
        put(o.llOn, a.s_pair, 0.0); put(o.llOff, a.s_pair, 0.0); put(o.mLogBQ, a.s_pair, 0.0);
        put(o.offHap, a.s_pair, (uint8_t)0); put(o.offHapHMQ, a.s_pair, (uint8_t)(status == DD_PAIR_OK ? 0 : 1));
        for (int16_t *f : {o.numIndels, o.numMismatch, o.nBQT, o.nmmBQT, o.nMMLeft, o.nMMRight}) put(f, a.s_pair, (int16_t)0);
        o.status[a.s_pair] = status;
        if (status != DD_PAIR_OK) {
            o.ll[a.s_pair] = 0.0;
            for (int i = 0; i < a.nv; i++) { put(o.var_covered, a.s_cov + i, (uint8_t)0); put(o.var_fcov, a.s_cov + i, (uint8_t)0); }
            continue;
        }
        fs_pair P;
        P.hap = b->hap_seq + hs; P.read = b->read_seq + so; P.qidx = b->read_qidx + so; P.T = T.data(); P.rel = rel;
        P.hlen = hlen; P.L = L; P.mqidx = b->read_mqidx[x.q];
        P.bMid = fs_bmid(b->win_hap_start[a.w], hlen, b->read_start[x.q], L);
        // votes and the diagonals
        const int nbins = fs_n_bins(hlen, L);
        for (int i = 0; i < nbins; i++) hist[(size_t)i] = 0;
        for (int k = 0; k < fs_n_read_kmers(L); k++) rk[(size_t)k] = (uint8_t)fs_kmer_key(P.read, k);
        for (int hx = 0; hx < fs_n_hap_kmers(hlen); hx++) fs_vote_hap_pos(P.hap, hx, rk.data(), L, hist.data());
        int n = 0;
        while (n < FS_MAX_DIAGONALS) {
            uint64_t best = 0;
            for (int i = 0; i < nbins; i++) best = std::max(best, fs_vote_rank(hist[(size_t)i], i));
            if (!best) break;
            const int bin = fs_rank_bin(best);
            rel[n++] = bin - L;
            hist[(size_t)bin] = 0;
        }
        P.S = fs_sort_diagonals(rel, n, L);
        const int T2 = 2 * P.S;
        // the two sweeps towards bMid
        for (int r = 0; r < P.bMid; r++) {
            for (int t = 0; t < T2; t++) {
                const fs_cell c = fs_left_step(&P, t, r, row[(r + 1) & 1]);
                row[r & 1][t] = c.v;
                bt[(size_t)r * FS_MAX_STATES + t] = (uint8_t)c.bp;
            }
            if (r == P.bMid - 1) memcpy(left, row[r & 1], sizeof(left));
        }
        for (int r = L - 1; r > P.bMid; r--) {
            for (int t = 0; t < T2; t++) {
                const fs_cell c = fs_right_step(&P, t, r, row[(r + 1) & 1]);
                row[r & 1][t] = c.v;
                bt[(size_t)r * FS_MAX_STATES + t] = (uint8_t)c.bp;
            }
            if (r == P.bMid + 1) memcpy(right, row[r & 1], sizeof(right));
        }
        // the join: plain '>' from minus infinity, the first maximum in state order
        double ll = -__builtin_huge_val(), mh = -__builtin_huge_val();
        int xmax = 0;
        for (int xx = 0; xx < T2; xx++) {
            const double v = fs_join(&P, xx, 0, left[xx], right[xx]), h = fs_join(&P, xx, 1, left[xx], right[xx]);
            if (v > ll) ll = v;
            if (h > mh) { mh = h; xmax = xx; }
        }
        fs_traceback(&P, bt.data(), xmax, path.data(), ms.data());
        int firstB = -1, lastB = -1;
        for (int r = 0; r < L; r++) {
            int hb;
            const int hp = fs_hpos_of(ms[(size_t)r], hlen, &hb);
            put(o.hpos, a.s_hpos + r, (int16_t)hp);
            if (hb >= 0) { firstB = firstB < 0 || hb < firstB ? hb : firstB; lastB = hb > lastB ? hb : lastB; }
        }
        for (int i = 0; i < a.nv; i++) {
            put(o.var_covered, a.s_cov + i,
                (uint8_t)fs_var_covered(firstB, lastB, p->padCover, b->hap_var[2 * (v0 + i)], b->hap_var[2 * (v0 + i) + 1]));
            if (!o.var_fcov || !b->hap_var_flank) continue;
            const int32_t *fl = b->hap_var_flank + 3 * (size_t)(v0 + i);
            const int lo = fl[0] - p->padCover, hi = fl[1] + p->padCover, kind = fl[2];
            int cov = 0;
            if (kind != 0 && hi >= lo) {
                memset(bits, 0, sizeof(bits));
                int nmm = 0, marked = 0;
                for (int r = 0; r < L; r++) nmm += fs_fcov_base(&P, ms.data(), r, lo, hi, kind, bits);
                for (int y = std::max(lo, 0); y <= std::min(hi, hlen - 1); y++) marked += fs_fcov_bit(bits, y);
                cov = marked >= hi - lo + 1 && nmm <= p->maxMismatch;
            }
            o.var_fcov[a.s_cov + i] = (uint8_t)cov;
        }
        o.ll[a.s_pair] = ll;
        put(o.firstBase, a.s_pair, (int16_t)firstB); put(o.lastBase, a.s_pair, (int16_t)lastB);
    }
    return DD_SUCCESS;
}

int dd_audit_compare_host_faster(const dd_batch *b, const dd_result *primary, const dd_audit_view *view, const dd_result *shadow, void *report,
                                 int64_t max_records)
{
    dd_sizes sz;
    int rc = dd_batch_sizes(b, &sz);
    if (rc) return rc;
    if (!primary || !shadow || !report) return fail(DD_ERR_INVALID, "dd_audit_compare_host_faster: null primary, shadow or report");
    if (max_records < 0) return fail(DD_ERR_INVALID, "dd_audit_compare_host_faster: negative max_records");
    if ((rc = check_audit_view("dd_audit_compare_host_faster", view, b->n_windows))) return rc;
    dd_audit_report *rep = static_cast<dd_audit_report *>(report);
    dd_audit_record *records = reinterpret_cast<dd_audit_record *>(rep + 1);
    memset(report, 0, DD_AUDIT_REPORT_BYTES(max_records));
    if (view->sizes.n_pairs == 0) return DD_SUCCESS;
    if (!primary->ll || !primary->status || !shadow->ll || !shadow->status)
        return fail(DD_ERR_INVALID, "dd_audit_compare_host_faster: ll and status are required on both sides");
    std::vector<int64_t> primary_off;
    au_geometry G;
    if ((rc = audit_geometry_host(b, view, primary_off, G))) return rc;
    const au_fields P = au_fields_of(primary), S = au_fields_of(shadow);
    const int has_flank = b->hap_var_flank != nullptr;
    for (int64_t j = 0; j < view->sizes.n_pairs; j++) {
        const au_pair a = au_locate(&G, j);
        const int st_p = (int)au_load(P.f[DD_AUDIT_FIELD_status], a.p_pair, 4), st_s = (int)au_load(S.f[DD_AUDIT_FIELD_status], a.s_pair, 4);
        rep->n_pairs++;
        const uint32_t open = st_p == st_s ? au_compared_faster(st_p, has_flank) : 1u << DD_AUDIT_FIELD_status;
        for (int f = 0; f < DD_AUDIT_N_FIELDS; f++) {
            if (!(open >> f & 1u) || !P.f[f] || !S.f[f]) continue;
            const int size = au_field_size(f);
            int64_t p0 = a.p_pair, s0 = a.s_pair;
            int n = 1;
            if (f == DD_AUDIT_FIELD_hpos) { p0 = a.p_hpos; s0 = a.s_hpos; n = a.L; }
            else if (f >= DD_AUDIT_N_PAIR_FIELDS) { p0 = a.p_cov; s0 = a.s_cov; n = a.nv; }
            rep->compared[f] += n;
            for (int i = 0; i < n; i++) {
                const uint64_t x = au_load(P.f[f], p0 + i, size), y = au_load(S.f[f], s0 + i, size);
                if (x == y) continue;
                rep->diff[f]++;
                if (rep->n_diff++ < max_records) records[rep->n_diff - 1] = {a.w, f, a.p_pair, p0 + i, x, y};
            }
        }
    }
    return DD_SUCCESS;
}

} // extern "C"
