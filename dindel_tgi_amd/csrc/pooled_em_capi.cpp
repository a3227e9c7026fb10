// pooled_em_capi.cpp — the device entries of the pooled analysis' EM loop (pooled_em_kernel.hip): the device-pointer launch and the
// host-pointer entry (its own allocation: one call per batch).  The CPU evaluation is pooled_em_host.cpp.
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
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(DD_ERR_NO_DEVICE, "no HIP device: dd_pooled_em runs on the device (dd_pooled_em_host is the CPU evaluation)");
    if (device < 0 || device >= ndev) return fail(DD_ERR_NO_DEVICE, "device ordinal out of range");
    HIP_TRY(hipSetDevice(device));
    if (N == 0) return DD_SUCCESS;
    const size_t F = (size_t)s->slot_off[N];

    // one allocation, 256-byte aligned pieces
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t o = off; off = (off + std::max<size_t>(bytes, 1) + 255u) & ~size_t(255u); return o; };
    const size_t o_ho = take((W + 1) * 4), o_ro = take((W + 1) * 4), o_po = take((W + 1) * 8), o_ll = take(n_pairs * 8), o_sw = take(N * 4),
                 o_so = take((N + 1) * 8), o_c = take(F), o_lk = take(N * 8), o_f = take(F * 8), o_it = take(N * 4), o_ed = take(N * 8);
    struct Mem {
        unsigned char *p = nullptr;
        ~Mem() { if (p) (void)hipFree(p); }
    } mem;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&mem.p), off));
    unsigned char *d = mem.p;
    auto up = [d](size_t o, const void *src, size_t bytes) { return bytes ? hipMemcpy(d + o, src, bytes, hipMemcpyHostToDevice) : hipSuccess; };
    HIP_TRY(up(o_ho, b->win_hap_off, (W + 1) * 4));
    HIP_TRY(up(o_ro, b->win_read_off, (W + 1) * 4));
    HIP_TRY(up(o_po, pair_off.data(), (W + 1) * 8));
    HIP_TRY(up(o_ll, ll_host, n_pairs * 8));
    HIP_TRY(up(o_sw, s->slot_window, N * 4));
    HIP_TRY(up(o_so, s->slot_off, (N + 1) * 8));
    HIP_TRY(up(o_c, s->compat, F));
    dd_device_batch db;
    memset(&db, 0, sizeof(db));
    db.n_windows = b->n_windows;
    db.win_hap_off = reinterpret_cast<const int32_t *>(d + o_ho); db.win_read_off = reinterpret_cast<const int32_t *>(d + o_ro);
    db.win_pair_off = reinterpret_cast<const int64_t *>(d + o_po);
    dd_pooled_slots ds = {s->n_slots, reinterpret_cast<const int32_t *>(d + o_sw), reinterpret_cast<const int64_t *>(d + o_so), d + o_c};
    dd_pooled_result dr = {reinterpret_cast<double *>(d + o_lk), reinterpret_cast<double *>(d + o_f), reinterpret_cast<int32_t *>(d + o_it),
                           reinterpret_cast<double *>(d + o_ed)};
    if ((rc = dd_pooled_em_device(&db, reinterpret_cast<const double *>(d + o_ll), &ds, max_haps, a0, tol, &dr, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    auto down = [d](void *dst, size_t o, size_t bytes) { return bytes ? hipMemcpy(dst, d + o, bytes, hipMemcpyDeviceToHost) : hipSuccess; };
    HIP_TRY(down(out->loglik, o_lk, N * 8));
    HIP_TRY(down(out->freqs, o_f, F * 8));
    HIP_TRY(down(out->iters, o_it, N * 4));
    HIP_TRY(down(out->ediff, o_ed, N * 8));
    return DD_SUCCESS;
}

} // extern "C"
