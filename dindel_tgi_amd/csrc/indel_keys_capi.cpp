// indel_keys_capi.cpp — the entries of the --faster model's indel-map key count (indel_keys_kernel.hip): the device-pointer launch, over
// the whole batch or a range of its pairs (the host-pointer entry, dd_compute_likelihoods_faster_keys, is a request of host_path.cpp's
// call), and the CPU evaluation from the same header (indel_keys_kernel.h), which makes no HIP call.
#include <thread>
#include "capi_internal.h"
#include "indel_keys_kernel.h"

namespace ddh {
int launch_indel_keys_range(const dd_device_batch *b, const int16_t *hpos_dev, const int32_t *status_dev, int16_t *out_dev, void *stream,
                            int64_t pair_begin, int64_t pair_end)
{
    if (!b || !hpos_dev || !out_dev) return fail(DD_ERR_INVALID, "dd_indel_keys_device: null batch, hpos or output array");
    if (b->n_windows < 0 || b->n_haps < 0 || b->n_reads < 0) return fail(DD_ERR_INVALID, "dd_indel_keys_device: negative count");
    if (pair_begin < 0) return fail(DD_ERR_INVALID, "dd_indel_keys_device: negative pair range");
    if (b->n_windows == 0 || b->n_haps == 0 || b->n_reads == 0 || (pair_end >= 0 && pair_end <= pair_begin)) return DD_SUCCESS;
    if (!b->win_read_off || !b->read_seq_off || !b->win_pair_off || !b->win_hpos_off) return fail(DD_ERR_INVALID, "dd_indel_keys_device: null offset array");
    ddi::IndelKeysArgs A;
    memset(&A, 0, sizeof(A));
    A.n_windows = b->n_windows;
    A.pair_begin = pair_begin; A.pair_end = pair_end;
    A.max_pairs = pair_end >= 0 ? pair_end - pair_begin : (int64_t)b->n_haps * b->n_reads;
    A.win_read_off = b->win_read_off; A.read_seq_off = b->read_seq_off; A.win_pair_off = b->win_pair_off; A.win_hpos_off = b->win_hpos_off;
    A.hpos = hpos_dev; A.pair_status = status_dev; A.out = out_dev;
    HIP_TRY(ddi::launch_indel_keys(A, static_cast<hipStream_t>(stream)));
    return DD_SUCCESS;
}
} // namespace ddh

using namespace ddh;

extern "C" {

int dd_indel_keys_device(const dd_device_batch *b, const int16_t *hpos_dev, const int32_t *status_dev, int16_t *out_dev, void *stream)
{
    return launch_indel_keys_range(b, hpos_dev, status_dev, out_dev, stream, 0, -1);
}

int dd_indel_keys_host(const dd_batch *b, const int16_t *hpos_host, const int32_t *status_host, int16_t *out, int nthreads)
{
    dd_sizes sz;
    const int rc = dd_batch_sizes(b, &sz);
    if (rc) return rc;
    if (sz.n_pairs == 0) return DD_SUCCESS;
    if (!hpos_host || !out) return fail(DD_ERR_INVALID, "dd_indel_keys_host: null hpos or output array");
    const int W = b->n_windows;
    std::vector<int64_t> pair_off((size_t)W + 1), hpos_off((size_t)W + 1);
    dd_batch_offsets(b, pair_off.data(), hpos_off.data(), nullptr);
    auto window = [&](int w) {
        const int q0 = b->win_read_off[w], R = b->win_read_off[w + 1] - q0, H = b->win_hap_off[w + 1] - b->win_hap_off[w];
        const int rs0 = b->read_seq_off[q0];
        const int64_t SL = (int64_t)b->read_seq_off[q0 + R] - rs0;
        for (int h = 0; h < H; h++)
            for (int r = 0; r < R; r++) {
                const int64_t pair = pair_off[(size_t)w] + (int64_t)h * R + r;
                const int rb = b->read_seq_off[q0 + r], L = b->read_seq_off[q0 + r + 1] - rb;
                if (status_host && status_host[pair] != DD_PAIR_OK) { out[pair] = DD_INDEL_KEYS_NOT_COMPUTED; continue; }   // hpos not read
                out[pair] = (int16_t)ik_count_serial(hpos_host + hpos_off[(size_t)w] + (int64_t)h * SL + (rb - rs0), L);
            }
    };
    const int nt = std::max(1, std::min(std::min(nthreads, W), 64));
    if (nt == 1) { for (int w = 0; w < W; w++) window(w); return DD_SUCCESS; }
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++) th.emplace_back([&, t]() { for (int w = t; w < W; w += nt) window(w); });
    for (auto &x : th) x.join();
    return DD_SUCCESS;
}

} // extern "C"
