// pooled_em_host.cpp — the pooled analysis' EM loop on the CPU (dd_pooled_em_host): pooled_math.h's loop over every slot, spread over
// host threads.  Plain C++ that builds with g++ alone (tests/pooled_em_check.cpp does; there no HIP header is read.  In the library the
// unit goes through hipcc like every other, and pooled_math.h then takes __host__ __device__ from the HIP runtime header): it is what
// the kernel's outputs are compared with bit for bit, and what callers without a device use.  Also the validation of a batch's slot
// tables, shared with the device entries.
#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <vector>
#include "../../include/dindel_hmm.h"
#include "pooled_math.h"

namespace ddh {
#ifdef DD_POOLED_EM_STANDALONE             // a program of this file alone (tests/pooled_em_check.cpp)
thread_local std::string g_err;
#else
extern thread_local std::string g_err;     // batch_host.cpp
#endif

int check_pooled_slots(const dd_batch *b, const dd_pooled_slots *s, double a0, double tol, const dd_pooled_result *out, int *max_haps_out)
{
    auto bad = [](const std::string &m) { g_err = m; return DD_ERR_INVALID; };
    if (!b || !s || !out) return bad("pooled EM: null batch, slots or result");
    if (b->n_windows < 0 || s->n_slots < 0) return bad("pooled EM: negative count");
    if (!(a0 > 0.0) || a0 > 1e300) return bad("pooled EM: a0 must be positive and finite");
    if (tol != tol) return bad("pooled EM: tol is not a number");
    if (b->n_windows > 0 && (!b->win_hap_off || !b->win_read_off)) return bad("pooled EM: null window offsets");
    for (int w = 0; w < b->n_windows; w++)
        if (b->win_hap_off[w + 1] < b->win_hap_off[w] || b->win_read_off[w + 1] < b->win_read_off[w])
            return bad("pooled EM: window offsets decrease at " + std::to_string(w));
    if (max_haps_out) *max_haps_out = 0;
    if (s->n_slots == 0) return DD_SUCCESS;
    if (!s->slot_window || !s->slot_off) return bad("pooled EM: null slot tables");
    if (!out->loglik || !out->iters || !out->ediff) return bad("pooled EM: null per-slot output");
    if (s->slot_off[0] != 0) return bad("pooled EM: slot_off does not start at 0");
    int mh = 0;
    for (int64_t i = 0; i < s->n_slots; i++) {
        const int w = s->slot_window[i];
        if (w < 0 || w >= b->n_windows) return bad("pooled EM: slot " + std::to_string(i) + " names no window of the batch");
        const int H = b->win_hap_off[w + 1] - b->win_hap_off[w];
        if (s->slot_off[i + 1] - s->slot_off[i] != H) return bad("pooled EM: slot " + std::to_string(i) + " does not own one entry per haplotype");
        if (H > mh) mh = H;
    }
    if (s->slot_off[s->n_slots] > 0 && (!s->compat || !out->freqs)) return bad("pooled EM: null compat or freqs");
    if (max_haps_out) *max_haps_out = mh;
    return DD_SUCCESS;
}
} // namespace ddh

extern "C" {

int dd_pooled_em_host(const dd_batch *b, const double *ll_host, const dd_pooled_slots *s, double a0, double tol, const dd_pooled_result *out,
                      int nthreads)
{
    int max_haps = 0;
    const int rc = ddh::check_pooled_slots(b, s, a0, tol, out, &max_haps);
    if (rc) return rc;
    if (s->n_slots == 0) return DD_SUCCESS;
    std::vector<int64_t> pair_off((size_t)b->n_windows + 1, 0);
    for (int w = 0; w < b->n_windows; w++)
        pair_off[w + 1] = pair_off[w] + (int64_t)(b->win_hap_off[w + 1] - b->win_hap_off[w]) * (b->win_read_off[w + 1] - b->win_read_off[w]);
    if (pair_off[b->n_windows] > 0 && !ll_host) { ddh::g_err = "pooled EM: null ll"; return DD_ERR_INVALID; }
    std::atomic<int64_t> next{0};
    auto work = [&]() {
        std::vector<double> w3((size_t)3 * (max_haps > 0 ? max_haps : 1));
        std::vector<PmSerialSum> nk((size_t)(max_haps > 0 ? max_haps : 1));
        for (int64_t i = next.fetch_add(1); i < s->n_slots; i = next.fetch_add(1)) {
            const int w = s->slot_window[i];
            const int H = b->win_hap_off[w + 1] - b->win_hap_off[w], R = b->win_read_off[w + 1] - b->win_read_off[w];
            const int64_t so = s->slot_off[i];
            pm_em_slot_serial(H, R, ll_host ? ll_host + pair_off[w] : nullptr, s->compat ? s->compat + so : nullptr, a0, tol, w3.data(),
                              w3.data() + max_haps, w3.data() + 2 * (size_t)max_haps, nk.data(), out->loglik + i,
                              out->freqs ? out->freqs + so : nullptr, out->iters + i, out->ediff + i);
        }
    };
    const int nt = (int)std::min<int64_t>(nthreads < 1 ? 1 : nthreads, s->n_slots);
    if (nt <= 1) { work(); return DD_SUCCESS; }
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; t++) pool.emplace_back(work);
    for (auto &t : pool) t.join();
    return DD_SUCCESS;
}

int dd_pooled_math_eval(int fn, const double *x, double *y, int64_t n)
{
    if (fn < 0 || fn > 3 || n < 0 || (n > 0 && (!x || !y))) { ddh::g_err = "dd_pooled_math_eval: bad argument"; return DD_ERR_INVALID; }
    for (int64_t i = 0; i < n; i++)
        y[i] = fn == 0 ? pm_exp(x[i]) : fn == 1 ? pm_log(x[i]) : fn == 2 ? pm_digamma(x[i]) : pm_add_logs(x[2 * i], x[2 * i + 1]);
    return DD_SUCCESS;
}

} // extern "C"
