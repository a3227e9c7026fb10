// diploid_pair_capi.cpp — the device entry of the certified MAP haplotype pair (diploid_pair_kernel.hip): the device-pointer launch, over the
// whole batch or a range of its windows (the host-pointer entry, dd_compute_likelihoods_realign_diploid, is a request of host_path.cpp's
// call).  The CPU evaluation is diploid_pair_host.cpp.
#include "capi_internal.h"
#include "diploid_pair_kernel.h"

namespace ddh {
int launch_diploid_pairs_range(const dd_device_batch *b, const int64_t *win_hh_off_dev, const double *ll_dev, const int32_t *status_dev,
                               const double *prior_dev, const dd_diploid_pair_result *out_dev, void *stream, int w0, int w1)
{
    if (!b || !out_dev) return fail(DD_ERR_INVALID, "dd_diploid_pairs_device: null batch or result");
    if (b->n_windows < 0) return fail(DD_ERR_INVALID, "dd_diploid_pairs_device: negative count");
    if (w1 < 0) w1 = b->n_windows;
    if (w0 < 0 || w1 > b->n_windows) return fail(DD_ERR_INVALID, "dd_diploid_pairs_device: window range outside the batch");
    if (w1 <= w0) return DD_SUCCESS;
    if (!b->win_hap_off || !b->win_read_off || !b->win_pair_off || !win_hh_off_dev || !ll_dev || !prior_dev || !out_dev->pair ||
        !out_dev->state || !out_dev->best || !out_dev->gap || !out_dev->margin)
        return fail(DD_ERR_INVALID, "dd_diploid_pairs_device: null array");
    ddq::DiploidPairArgs A;
    // the offsets hold positions in the whole batch's arrays: a range is the same launch with the per-window arrays started at w0
    A.n_windows = w1 - w0;
    A.win_hap_off = b->win_hap_off + w0; A.win_read_off = b->win_read_off + w0; A.win_pair_off = b->win_pair_off + w0; A.win_hh_off = win_hh_off_dev + w0;
    A.ll = ll_dev; A.prior = prior_dev; A.status = status_dev;
    A.out = {out_dev->pair + 2 * (size_t)w0, out_dev->state + w0, out_dev->best + w0, out_dev->gap + w0, out_dev->margin + w0};
    HIP_TRY(ddq::launch_diploid_pairs(A, static_cast<hipStream_t>(stream)));
    return DD_SUCCESS;
}
} // namespace ddh

using namespace ddh;

extern "C" {

int dd_diploid_pairs_device(const dd_device_batch *b, const int64_t *win_hh_off_dev, const double *ll_dev, const int32_t *status_dev,
                            const double *prior_dev, const dd_diploid_pair_result *out_dev, void *stream)
{
    return launch_diploid_pairs_range(b, win_hh_off_dev, ll_dev, status_dev, prior_dev, out_dev, stream, 0, -1);
}

} // extern "C"
