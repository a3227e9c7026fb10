// hapdist_host.cpp — host side of the block table (hapdist_kernel.hip): validation of a dd_hap_batch and of the caller's capacities, the
// capacity rule (dd_hap_blocks_offsets), the device-pointer launch and the host-pointer entry (its own allocation: one call per batch of
// windows).
#include "capi_internal.h"
#include "hapdist_kernel.h"

namespace ddh {
namespace {

struct HapShape { int64_t ref_bytes, n_ops, n_bases; };

// this thread's last launch; its two device words are read on demand, or cached by the host entry (whose workspace goes with the call)
struct HapLast { int64_t v[DD_HAP_BLOCKS_LOG_FIELDS]; const unsigned char *ws; hipStream_t stream; bool have_stats; };
thread_local HapLast g_hap_last = {{0, 0, 0, 0}, nullptr, nullptr, true};

int read_hap_stats()
{
    HapLast &L = g_hap_last;
    if (L.have_stats || !L.ws) return DD_SUCCESS;
    uint32_t hdr[3];
    HIP_TRY(hipStreamSynchronize(L.stream));
    HIP_TRY(hipMemcpy(hdr, L.ws, sizeof(hdr), hipMemcpyDeviceToHost));
    L.v[2] = hdr[DD_HAPDIST_HDR_MAX_DRAWS]; L.v[3] = hdr[DD_HAPDIST_HDR_TRIPS];
    L.have_stats = true;
    return DD_SUCCESS;
}

int check_offsets(const int32_t *off, int64_t n, const char *name)
{
    if (!off) return fail(DD_ERR_INVALID, std::string("null ") + name + " in hap batch");
    if (off[0] != 0) return fail(DD_ERR_INVALID, std::string(name) + " does not start at 0");
    for (int64_t i = 0; i < n; i++)
        if (off[i + 1] < off[i]) return fail(DD_ERR_INVALID, std::string(name) + " decreases at " + std::to_string(i));
    return DD_SUCCESS;
}

// offsets start at 0 and never decrease; the windows' read ranges end at n_reads.  What a read holds (positions, operations, letters) is
// the kernel's to judge: it decides a window's status.
int check_hap_batch(const dd_hap_batch *b, HapShape &s)
{
    if (!b) return fail(DD_ERR_INVALID, "null hap batch");
    if (b->n_windows < 0 || b->n_reads < 0) return fail(DD_ERR_INVALID, "negative count in hap batch");
    int rc;
    if ((rc = check_offsets(b->win_ref_off, b->n_windows, "win_ref_off"))) return rc;
    if ((rc = check_offsets(b->win_read_off, b->n_windows, "win_read_off"))) return rc;
    if ((rc = check_offsets(b->read_op_off, b->n_reads, "read_op_off"))) return rc;
    if ((rc = check_offsets(b->read_base_off, b->n_reads, "read_base_off"))) return rc;
    if (b->win_read_off[b->n_windows] != b->n_reads) return fail(DD_ERR_INVALID, "win_read_off does not end at n_reads");
    s.ref_bytes = b->win_ref_off[b->n_windows]; s.n_ops = b->read_op_off[b->n_reads]; s.n_bases = b->read_base_off[b->n_reads];
    if (b->n_windows > 0 && !b->win_rs) return fail(DD_ERR_INVALID, "null win_rs in hap batch");
    if (b->n_reads > 0 && (!b->read_pos || !b->read_flag)) return fail(DD_ERR_INVALID, "null read_pos or read_flag in hap batch");
    if (s.ref_bytes > 0 && !b->ref_seq) return fail(DD_ERR_INVALID, "null ref_seq in hap batch");
    if (s.n_ops > 0 && !b->ops) return fail(DD_ERR_INVALID, "null ops in hap batch");
    if (s.n_bases > 0 && !b->bases) return fail(DD_ERR_INVALID, "null bases in hap batch");
    return DD_SUCCESS;
}

} // namespace
} // namespace ddh

using namespace ddh;

extern "C" {

int dd_hap_blocks_offsets(const dd_hap_batch *b, int32_t *blk_off, int32_t *ent_off, int32_t *ins_off)
{
    HapShape s;
    int rc = check_hap_batch(b, s);
    if (rc) return rc;
    if (!blk_off || !ent_off || !ins_off) return fail(DD_ERR_INVALID, "dd_hap_blocks_offsets: null output");
    int64_t nb = 0, ne = 0, ni = 0;
    blk_off[0] = ent_off[0] = ins_off[0] = 0;
    for (int w = 0; w < b->n_windows; w++) {
        const int64_t L = (int64_t)b->win_ref_off[w + 1] - b->win_ref_off[w];
        if (L <= DD_HAPDIST_MAX_WINDOW) { nb += L; ne += 4 * L + 64; }
        for (int r = b->win_read_off[w]; r < b->win_read_off[w + 1]; r++)
            for (int k = b->read_op_off[r]; k < b->read_op_off[r + 1]; k++) ni += (b->ops[k] & 15u) == 1u;
        if (nb > INT32_MAX || ne > INT32_MAX || ni > INT32_MAX) return fail(DD_ERR_INVALID, "dd_hap_blocks_offsets: the batch's tables exceed 2^31 words");
        blk_off[w + 1] = (int32_t)nb; ent_off[w + 1] = (int32_t)ne; ins_off[w + 1] = (int32_t)ni;
    }
    return DD_SUCCESS;
}

size_t dd_hap_blocks_workspace_bytes(void) { return DD_HAPDIST_WS_BYTES; }

int dd_hap_blocks_device(const dd_hap_batch *b, const dd_hap_blocks *t, int64_t max_blk, int64_t max_ent, int64_t max_ins, void *workspace,
                         size_t workspace_bytes, void *stream)
{
    if (!b || !t) return fail(DD_ERR_INVALID, "dd_hap_blocks_device: null batch or tables");
    if (b->n_windows < 0 || b->n_reads < 0) return fail(DD_ERR_INVALID, "dd_hap_blocks_device: negative count");
    if (max_blk < 0 || max_ent < 0 || max_ins < 0) return fail(DD_ERR_INVALID, "dd_hap_blocks_device: negative capacity");
    if (b->n_windows == 0) return DD_SUCCESS;
    if (!b->win_rs || !b->win_ref_off || !b->ref_seq || !b->win_read_off || !b->read_pos || !b->read_flag || !b->read_op_off || !b->ops ||
        !b->read_base_off || !b->bases)
        return fail(DD_ERR_INVALID, "dd_hap_blocks_device: null array in the batch");
    if (!t->status || !t->n_blocks || !t->n_entries || !t->n_ins_ops || !t->n_ins_pos || !t->left || !t->blk_off || !t->ent_off || !t->ins_off ||
        !t->blocks || !t->entries || !t->ins_ops || !t->ins_pos)
        return fail(DD_ERR_INVALID, "dd_hap_blocks_device: null array in the tables");
    if (reinterpret_cast<uintptr_t>(t->entries) & 7u) return fail(DD_ERR_INVALID, "dd_hap_blocks_device: entries must be 8-byte aligned");
    if (!workspace || workspace_bytes < DD_HAPDIST_WS_BYTES)
        return fail(DD_ERR_INVALID, "dd_hap_blocks_device: workspace missing or too small (dd_hap_blocks_workspace_bytes)");
    dda::HapdistArgs A;
    A.b = *b; A.t = *t;
    A.max_blk = max_blk; A.max_ent = max_ent; A.max_ins = max_ins;
    A.hdr = static_cast<unsigned int *>(workspace);
    const int64_t rec[DD_HAP_BLOCKS_LOG_FIELDS] = {(int64_t)dda::hapdist_grid(b->n_windows), (int64_t)b->n_windows, -1, -1};
    memcpy(g_hap_last.v, rec, sizeof(rec));
    g_hap_last.ws = static_cast<const unsigned char *>(workspace); g_hap_last.stream = static_cast<hipStream_t>(stream);
    g_hap_last.have_stats = false;
    HIP_TRY(dda::launch_hapdist(A, static_cast<hipStream_t>(stream)));
    return DD_SUCCESS;
}

void dd_hap_blocks_last_launch(int64_t out[DD_HAP_BLOCKS_LOG_FIELDS])
{
    (void)read_hap_stats();                    // a failure leaves -1 in the two device fields
    if (out) memcpy(out, g_hap_last.v, sizeof(g_hap_last.v));
}

int dd_hap_blocks_compute(const dd_hap_batch *b, dd_hap_blocks *t, int device)
{
    HapShape s;
    int rc = check_hap_batch(b, s);
    if (rc) return rc;
    if (!t) return fail(DD_ERR_INVALID, "null hap tables");
    const size_t W = (size_t)b->n_windows, R = (size_t)b->n_reads;
    if (W > 0 && (!t->status || !t->n_blocks || !t->n_entries || !t->n_ins_ops || !t->n_ins_pos || !t->left))
        return fail(DD_ERR_INVALID, "null per-window array in hap tables");
    if (!t->blk_off || !t->ent_off || !t->ins_off) return fail(DD_ERR_INVALID, "null capacity offsets in hap tables");
    const int32_t *offs[3] = {t->blk_off, t->ent_off, t->ins_off};
    const char *names[3] = {"blk_off", "ent_off", "ins_off"};
    for (int i = 0; i < 3; i++) {
        if (offs[i][0] != 0) return fail(DD_ERR_INVALID, std::string(names[i]) + " does not start at 0");
        for (size_t w = 0; w < W; w++)
            if (offs[i][w + 1] < offs[i][w]) return fail(DD_ERR_INVALID, std::string(names[i]) + " decreases at window " + std::to_string(w));
    }
    const size_t n_blk = (size_t)t->blk_off[W], n_ent = (size_t)t->ent_off[W], n_ins = (size_t)t->ins_off[W];
    if ((n_blk && !t->blocks) || (n_ent && !t->entries) || (n_ins && (!t->ins_ops || !t->ins_pos)))
        return fail(DD_ERR_INVALID, "null table in hap tables");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(DD_ERR_NO_DEVICE, "no HIP device: the library's block table runs on the device (host/haplotypes.cpp holds the host twin)");
    if (device < 0 || device >= ndev) return fail(DD_ERR_NO_DEVICE, "device ordinal out of range");
    HIP_TRY(hipSetDevice(device));
    if (W == 0) return DD_SUCCESS;

    // one allocation, 256-byte aligned pieces: inputs, per-window outputs, tables, workspace
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t o = off; off = (off + std::max<size_t>(bytes, 1) + 255u) & ~size_t(255u); return o; };
    const size_t o_rs = take(W * 4), o_refo = take((W + 1) * 4), o_ref = take((size_t)s.ref_bytes), o_wro = take((W + 1) * 4),
                 o_pos = take(R * 4), o_flag = take(R * 4), o_opo = take((R + 1) * 4), o_ops = take((size_t)s.n_ops * 4),
                 o_bo = take((R + 1) * 4), o_bases = take((size_t)s.n_bases), o_in_end = off;
    const size_t o_win = take(6 * W * 4), o_blko = take((W + 1) * 4), o_ento = take((W + 1) * 4), o_inso = take((W + 1) * 4),
                 o_blk = take(n_blk * 4), o_ent = take(n_ent * 8), o_iops = take(n_ins * 8), o_ipos = take(n_ins * 8),
                 o_ws = take(DD_HAPDIST_WS_BYTES);
    (void)o_in_end;
    struct Mem {
        unsigned char *p = nullptr;
        ~Mem() { if (p) (void)hipFree(p); }
    } mem;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&mem.p), off));
    unsigned char *d = mem.p;
    auto up = [d](size_t o, const void *src, size_t bytes) { return bytes ? hipMemcpy(d + o, src, bytes, hipMemcpyHostToDevice) : hipSuccess; };
    HIP_TRY(up(o_rs, b->win_rs, W * 4));
    HIP_TRY(up(o_refo, b->win_ref_off, (W + 1) * 4));
    HIP_TRY(up(o_ref, b->ref_seq, (size_t)s.ref_bytes));
    HIP_TRY(up(o_wro, b->win_read_off, (W + 1) * 4));
    HIP_TRY(up(o_pos, b->read_pos, R * 4));
    HIP_TRY(up(o_flag, b->read_flag, R * 4));
    HIP_TRY(up(o_opo, b->read_op_off, (R + 1) * 4));
    HIP_TRY(up(o_ops, b->ops, (size_t)s.n_ops * 4));
    HIP_TRY(up(o_bo, b->read_base_off, (R + 1) * 4));
    HIP_TRY(up(o_bases, b->bases, (size_t)s.n_bases));
    HIP_TRY(up(o_blko, t->blk_off, (W + 1) * 4));
    HIP_TRY(up(o_ento, t->ent_off, (W + 1) * 4));
    HIP_TRY(up(o_inso, t->ins_off, (W + 1) * 4));
    dd_hap_batch db = *b;
    db.win_rs = reinterpret_cast<const int32_t *>(d + o_rs); db.win_ref_off = reinterpret_cast<const int32_t *>(d + o_refo);
    db.ref_seq = reinterpret_cast<const char *>(d + o_ref); db.win_read_off = reinterpret_cast<const int32_t *>(d + o_wro);
    db.read_pos = reinterpret_cast<const int32_t *>(d + o_pos); db.read_flag = reinterpret_cast<const int32_t *>(d + o_flag);
    db.read_op_off = reinterpret_cast<const int32_t *>(d + o_opo); db.ops = reinterpret_cast<const uint32_t *>(d + o_ops);
    db.read_base_off = reinterpret_cast<const int32_t *>(d + o_bo); db.bases = reinterpret_cast<const char *>(d + o_bases);
    int32_t *dw = reinterpret_cast<int32_t *>(d + o_win);
    dd_hap_blocks dt;
    dt.status = dw; dt.n_blocks = dw + W; dt.n_entries = dw + 2 * W; dt.n_ins_ops = dw + 3 * W; dt.n_ins_pos = dw + 4 * W; dt.left = dw + 5 * W;
    dt.blk_off = reinterpret_cast<const int32_t *>(d + o_blko); dt.ent_off = reinterpret_cast<const int32_t *>(d + o_ento);
    dt.ins_off = reinterpret_cast<const int32_t *>(d + o_inso);
    dt.blocks = reinterpret_cast<uint32_t *>(d + o_blk); dt.entries = reinterpret_cast<uint32_t *>(d + o_ent);
    dt.ins_ops = reinterpret_cast<uint32_t *>(d + o_iops); dt.ins_pos = reinterpret_cast<uint32_t *>(d + o_ipos);
    // what the kernel leaves alone comes back as the caller had it
    HIP_TRY(up(o_win, t->status, W * 4)); HIP_TRY(up(o_win + W * 4, t->n_blocks, W * 4)); HIP_TRY(up(o_win + 2 * W * 4, t->n_entries, W * 4));
    HIP_TRY(up(o_win + 3 * W * 4, t->n_ins_ops, W * 4)); HIP_TRY(up(o_win + 4 * W * 4, t->n_ins_pos, W * 4)); HIP_TRY(up(o_win + 5 * W * 4, t->left, W * 4));
    HIP_TRY(up(o_blk, t->blocks, n_blk * 4)); HIP_TRY(up(o_ent, t->entries, n_ent * 8));
    HIP_TRY(up(o_iops, t->ins_ops, n_ins * 8)); HIP_TRY(up(o_ipos, t->ins_pos, n_ins * 8));
    if ((rc = dd_hap_blocks_device(&db, &dt, (int64_t)n_blk, (int64_t)n_ent, (int64_t)n_ins, d + o_ws, DD_HAPDIST_WS_BYTES, nullptr))) {
        g_hap_last.ws = nullptr;
        return rc;
    }
    HIP_TRY(hipStreamSynchronize(nullptr));
    if ((rc = read_hap_stats())) return rc;    // the workspace goes with this call
    g_hap_last.ws = nullptr;
    auto down = [d](void *dst, size_t o, size_t bytes) { return bytes ? hipMemcpy(dst, d + o, bytes, hipMemcpyDeviceToHost) : hipSuccess; };
    HIP_TRY(down(t->status, o_win, W * 4)); HIP_TRY(down(t->n_blocks, o_win + W * 4, W * 4)); HIP_TRY(down(t->n_entries, o_win + 2 * W * 4, W * 4));
    HIP_TRY(down(t->n_ins_ops, o_win + 3 * W * 4, W * 4)); HIP_TRY(down(t->n_ins_pos, o_win + 4 * W * 4, W * 4)); HIP_TRY(down(t->left, o_win + 5 * W * 4, W * 4));
    HIP_TRY(down(t->blocks, o_blk, n_blk * 4)); HIP_TRY(down(t->entries, o_ent, n_ent * 8));
    HIP_TRY(down(t->ins_ops, o_iops, n_ins * 8)); HIP_TRY(down(t->ins_pos, o_ipos, n_ins * 8));
    return DD_SUCCESS;
}

} // extern "C"
