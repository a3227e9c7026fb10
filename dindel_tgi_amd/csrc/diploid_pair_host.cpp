// diploid_pair_host.cpp — the certified MAP haplotype pair on the CPU (dd_diploid_pairs_host): diploid_pair_kernel.h's function over every
// window, spread over host threads.  Plain C++ that builds with g++ alone (tests/diploid_pair_check.cpp does; in the library the unit goes
// through hipcc like every other): it is what the kernel's outputs are compared with bit for bit, and what callers without a device use.
// Also the validation of a batch's arrays, shared with the device entries.
#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <vector>
#include "diploid_pair_kernel.h"

namespace ddh {
#ifdef DD_DIPLOID_PAIR_STANDALONE          // a program of this file alone (tests/diploid_pair_check.cpp)
thread_local std::string g_err;
#else
extern thread_local std::string g_err;     // batch_host.cpp
#endif

int check_diploid_pairs(const dd_batch *b, const double *ll, const double *prior, const dd_diploid_pair_result *out)
{
    auto bad = [](const std::string &m) { g_err = m; return DD_ERR_INVALID; };
    if (!b || !out) return bad("diploid pairs: null batch or result");
    if (b->n_windows < 0) return bad("diploid pairs: negative count");
    if (b->n_windows == 0) return DD_SUCCESS;
    if (!b->win_hap_off || !b->win_read_off) return bad("diploid pairs: null window offsets");
    if (!out->pair || !out->state || !out->best || !out->gap || !out->margin) return bad("diploid pairs: every array of dd_diploid_pair_result is required");
    int64_t n_pairs = 0, n_hh = 0;
    for (int w = 0; w < b->n_windows; w++) {
        const int64_t H = (int64_t)b->win_hap_off[w + 1] - b->win_hap_off[w], R = (int64_t)b->win_read_off[w + 1] - b->win_read_off[w];
        if (H < 0 || R < 0) return bad("diploid pairs: window offsets decrease at " + std::to_string(w));
        n_pairs += H * R; n_hh += H * H;
    }
    if (n_pairs > 0 && !ll) return bad("diploid pairs: null ll");
    if (n_hh > 0 && !prior) return bad("diploid pairs: null prior");
    return DD_SUCCESS;
}
} // namespace ddh

extern "C" {

int dd_diploid_pairs_host(const dd_batch *b, const double *ll_host, const int32_t *status_host, const double *prior_host,
                          const dd_diploid_pair_result *out, int nthreads)
{
    const int rc = ddh::check_diploid_pairs(b, ll_host, prior_host, out);
    if (rc) return rc;
    const int W = b->n_windows;
    if (W == 0) return DD_SUCCESS;
    std::vector<int64_t> pair_off((size_t)W + 1, 0), hh_off((size_t)W + 1, 0);
    for (int w = 0; w < W; w++) {
        const int64_t H = b->win_hap_off[w + 1] - b->win_hap_off[w], R = b->win_read_off[w + 1] - b->win_read_off[w];
        pair_off[w + 1] = pair_off[w] + H * R;
        hh_off[w + 1] = hh_off[w] + H * H;
    }
    const double log_half = pm_log(0.5);
    std::atomic<int> next{0};
    auto work = [&]() {
        for (int w = next.fetch_add(1); w < W; w = next.fetch_add(1)) {
            const int H = b->win_hap_off[w + 1] - b->win_hap_off[w], R = b->win_read_off[w + 1] - b->win_read_off[w];
            const double *ll = ll_host ? ll_host + pair_off[w] : nullptr;
            int early = DD_DIPPAIR_CERTIFIED;
            if (H <= 0) {
                early = DD_DIPPAIR_NO_HAPS;
            } else if (H > DD_DIPPAIR_MAX_HAPS) {
                early = DD_DIPPAIR_TOO_MANY_HAPS;
            } else {
                const int32_t *status = status_host ? status_host + pair_off[w] : nullptr;
                bool bad_status = false, bad_ll = false;
                for (int64_t i = 0; i < (int64_t)H * R; i++) {
                    if (status && status[i] != 0) bad_status = true;
                    if (!dp_finite(ll[i])) bad_ll = true;
                }
                if (bad_status) early = DD_DIPPAIR_NOT_COMPUTED;
                else if (bad_ll) early = DD_DIPPAIR_NONFINITE;
            }
            DpTop2 top;
            dp_top2_clear(top);
            bool any_nan = false;
            if (early == DD_DIPPAIR_CERTIFIED) {
                const double *prior = prior_host + hh_off[w];
                int p = 0;
                for (int h1 = 0; h1 < H; h1++)
                    for (int h2 = h1; h2 < H; h2++, p++) {
                        DpAcc acc;
                        dp_acc_clear(acc);
                        for (int r = 0; r < R; r++) dp_acc_add(acc, ll[(int64_t)h1 * R + r], ll[(int64_t)h2 * R + r], log_half);
                        double V, eps;
                        dp_value(acc, R, prior[(int64_t)h1 * H + h2], V, eps);
                        if (V != V) any_nan = true;
                        dp_top2_offer(top, V, eps, p);
                    }
            }
            dp_finish(H, early, any_nan, top, out->pair + 2 * (int64_t)w, out->state + w, out->best + w, out->gap + w, out->margin + w);
        }
    };
    const int nt = std::min(nthreads < 1 ? 1 : nthreads, W);
    if (nt <= 1) { work(); return DD_SUCCESS; }
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; t++) pool.emplace_back(work);
    for (auto &t : pool) t.join();
    return DD_SUCCESS;
}

} // extern "C"
