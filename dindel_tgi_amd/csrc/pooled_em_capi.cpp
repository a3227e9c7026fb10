// pooled_em_capi.cpp — the device entries of the pooled analysis' EM loop (pooled_em_kernel.hip): the device-pointer launch and the
// host-pointer entry: its checks and its list of arrays (the arena and the copy back are capi_internal.h's).  The CPU evaluation is
// pooled_em_host.cpp.
#include "capi_internal.h"
#include "pooled_em_kernel.h"

using namespace ddh;

extern "C" {

int dd_pooled_em_device(const dd_device_batch *b, const double *ll_dev, const dd_pooled_slots *s_dev, int max_haps, double a0, double tol,
                        const dd_pooled_result *out_dev, void *stream)
{
    if (!b || !s_dev || !out_dev) return fail(DD_ERR_INVALID, "dd_pooled_em_device: null batch, slots or result");
    if (b->n_windows < 0 || s_dev->n_slots < 0) return fail(DD_ERR_INVALID, "dd_pooled_em_device: negative count");
    if (!(a0 > 0.0) || a0 > 1e300 || tol != tol) return fail(DD_ERR_INVALID, "dd_pooled_em_device: a0 must be positive and finite, tol a number");
    if (max_haps < 0 || max_haps > DD_POOLED_MAX_HAPS) return fail(DD_ERR_UNSUPPORTED, "dd_pooled_em_device: max_haps outside [0, DD_POOLED_MAX_HAPS]");
    if (s_dev->n_slots == 0) return DD_SUCCESS;
    if (s_dev->n_slots > 0x7fffffffLL) return fail(DD_ERR_UNSUPPORTED, "dd_pooled_em_device: too many slots for one launch");
    if (!b->win_hap_off || !b->win_read_off || !b->win_pair_off || !ll_dev || !s_dev->slot_window || !s_dev->slot_off || !s_dev->compat ||
        !out_dev->loglik || !out_dev->freqs || !out_dev->iters || !out_dev->ediff)
        return fail(DD_ERR_INVALID, "dd_pooled_em_device: null array");
    ddp::PooledEmArgs A;
    A.n_windows = b->n_windows; A.max_haps = max_haps; A.n_slots = s_dev->n_slots;
    A.win_hap_off = b->win_hap_off; A.win_read_off = b->win_read_off; A.win_pair_off = b->win_pair_off;
    A.ll = ll_dev; A.s = *s_dev; A.out = *out_dev; A.a0 = a0; A.tol = tol;
    HIP_TRY(ddp::launch_pooled_em(A, static_cast<hipStream_t>(stream)));
    return DD_SUCCESS;
}

int dd_pooled_em(const dd_batch *b, const double *ll_host, const dd_pooled_slots *s, double a0, double tol, const dd_pooled_result *out,
                 int device)
{
    int max_haps = 0;
    int rc = check_pooled_slots(b, s, a0, tol, out, &max_haps);
    if (rc) return rc;
    if (max_haps > DD_POOLED_MAX_HAPS) return fail(DD_ERR_UNSUPPORTED, "dd_pooled_em: a window has more than DD_POOLED_MAX_HAPS haplotypes");
    const size_t W = (size_t)b->n_windows, N = (size_t)s->n_slots;
    std::vector<int64_t> pair_off(W + 1, 0);
    for (size_t w = 0; w < W; w++)
        pair_off[w + 1] = pair_off[w] + (int64_t)(b->win_hap_off[w + 1] - b->win_hap_off[w]) * (b->win_read_off[w + 1] - b->win_read_off[w]);
    const size_t n_pairs = (size_t)pair_off[W];
    if (n_pairs > 0 && !ll_host) return fail(DD_ERR_INVALID, "dd_pooled_em: null ll");
    if ((rc = use_device(device, "no HIP device: dd_pooled_em runs on the device (dd_pooled_em_host is the CPU evaluation)"))) return rc;
    if (N == 0) return DD_SUCCESS;
    const size_t F = (size_t)s->slot_off[N];

    // every array of the call once: the window offsets, the likelihoods, the slot tables and the four outputs
    dd_device_batch db;
    memset(&db, 0, sizeof(db));
    db.n_windows = b->n_windows;
    const double *d_ll;
    dd_pooled_slots ds = *s;
    dd_pooled_result dr;
    OneShotArena arena;
    if ((rc = arena.place({arena_slot(&db.win_hap_off, (W + 1) * 4, b->win_hap_off), arena_slot(&db.win_read_off, (W + 1) * 4, b->win_read_off),
                           arena_slot(&db.win_pair_off, (W + 1) * 8, pair_off.data()), arena_slot(&d_ll, n_pairs * 8, ll_host),
                           arena_slot(&ds.slot_window, N * 4, s->slot_window), arena_slot(&ds.slot_off, (N + 1) * 8, s->slot_off),
                           arena_slot(&ds.compat, F, s->compat), arena_slot(&dr.loglik, N * 8), arena_slot(&dr.freqs, F * 8),
                           arena_slot(&dr.iters, N * 4), arena_slot(&dr.ediff, N * 8)})))
        return rc;
    if ((rc = dd_pooled_em_device(&db, d_ll, &ds, max_haps, a0, tol, &dr, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return download({{out->loglik, dr.loglik, N * 8}, {out->freqs, dr.freqs, F * 8}, {out->iters, dr.iters, N * 4}, {out->ediff, dr.ediff, N * 8}});
}

} // extern "C"
