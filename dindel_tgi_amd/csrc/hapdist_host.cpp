// hapdist_host.cpp — host side of the block table (hapdist_kernel.hip): validation of a dd_hap_batch and of the caller's capacities, the
// capacity rule (dd_hap_blocks_offsets), the device-pointer launch with its launch record, and the host-pointer entry: its checks and its
// list of arrays.  The arena, the record and the copy back are capi_internal.h's.
#include "capi_internal.h"
#include "hapdist_kernel.h"

namespace ddh {
namespace {

struct HapShape { int64_t ref_bytes, n_ops, n_bases; };

thread_local LaunchRecord g_hap_last(DD_HAP_BLOCKS_LOG_FIELDS);   // this thread's last launch (capi_internal.h)

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
    g_hap_last.note({(int64_t)dda::persistent_grid(b->n_windows, DD_HAPDIST_WAVES, DD_HAPDIST_MAX_BLOCKS), (int64_t)b->n_windows}, workspace,
                     DD_HAPDIST_HDR_BASE, stream);
    HIP_TRY(dda::launch_hapdist(A, static_cast<hipStream_t>(stream)));
    return DD_SUCCESS;
}

void dd_hap_blocks_last_launch(int64_t out[DD_HAP_BLOCKS_LOG_FIELDS]) { g_hap_last.copy_out(out); }

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
    if ((rc = use_device(device, "no HIP device: the library's block table runs on the device (host/haplotypes.cpp holds the host twin)"))) return rc;
    if (W == 0) return DD_SUCCESS;

    // every array of the call once: the batch, the capacities, and the tables, which go up as well as down (what the kernel leaves alone
    // comes back as the caller had it), and the workspace
    const size_t ref_bytes = (size_t)s.ref_bytes, n_ops = (size_t)s.n_ops, n_bases = (size_t)s.n_bases;
    dd_hap_batch db = *b;
    dd_hap_blocks dt;
    unsigned char *ws;
    OneShotArena arena;
    ArenaRecords records(arena, {&g_hap_last});
    if ((rc = arena.place({arena_slot(&db.win_rs, W * 4, b->win_rs), arena_slot(&db.win_ref_off, (W + 1) * 4, b->win_ref_off),
                           arena_slot(&db.ref_seq, ref_bytes, b->ref_seq), arena_slot(&db.win_read_off, (W + 1) * 4, b->win_read_off),
                           arena_slot(&db.read_pos, R * 4, b->read_pos), arena_slot(&db.read_flag, R * 4, b->read_flag),
                           arena_slot(&db.read_op_off, (R + 1) * 4, b->read_op_off), arena_slot(&db.ops, n_ops * 4, b->ops),
                           arena_slot(&db.read_base_off, (R + 1) * 4, b->read_base_off), arena_slot(&db.bases, n_bases, b->bases),
                           arena_slot(&dt.status, W * 4, t->status), arena_slot(&dt.n_blocks, W * 4, t->n_blocks),
                           arena_slot(&dt.n_entries, W * 4, t->n_entries), arena_slot(&dt.n_ins_ops, W * 4, t->n_ins_ops),
                           arena_slot(&dt.n_ins_pos, W * 4, t->n_ins_pos), arena_slot(&dt.left, W * 4, t->left),
                           arena_slot(&dt.blk_off, (W + 1) * 4, t->blk_off), arena_slot(&dt.ent_off, (W + 1) * 4, t->ent_off),
                           arena_slot(&dt.ins_off, (W + 1) * 4, t->ins_off), arena_slot(&dt.blocks, n_blk * 4, t->blocks),
                           arena_slot(&dt.entries, n_ent * 8, t->entries), arena_slot(&dt.ins_ops, n_ins * 8, t->ins_ops),
                           arena_slot(&dt.ins_pos, n_ins * 8, t->ins_pos), arena_slot(&ws, DD_HAPDIST_WS_BYTES)})))
        return rc;
    if ((rc = dd_hap_blocks_device(&db, &dt, (int64_t)n_blk, (int64_t)n_ent, (int64_t)n_ins, ws, DD_HAPDIST_WS_BYTES, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    if ((rc = records.read_stats())) return rc;   // the workspace goes with this call
    return download({{t->status, dt.status, W * 4}, {t->n_blocks, dt.n_blocks, W * 4}, {t->n_entries, dt.n_entries, W * 4},
                     {t->n_ins_ops, dt.n_ins_ops, W * 4}, {t->n_ins_pos, dt.n_ins_pos, W * 4}, {t->left, dt.left, W * 4},
                     {t->blocks, dt.blocks, n_blk * 4}, {t->entries, dt.entries, n_ent * 8}, {t->ins_ops, dt.ins_ops, n_ins * 8},
                     {t->ins_pos, dt.ins_pos, n_ins * 8}});
}

} // extern "C"
