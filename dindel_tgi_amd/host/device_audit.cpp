// device_audit.cpp — LikelihoodEngine::setAudit and setAuditFaster: the switches, and the one place of the adapter that names the C ABI's
// audit entries (dd_audit_select, dd_compute_likelihoods_audit, their --faster counterparts and the library's test hook).  runBatch calls
// auditedCall / auditedFasterCall through the pointers set here (as device_indel_keys.cpp does for its entry: a program that stubs the C
// ABI without these entries and never sets the switches links).
#include "compute_likelihoods.hpp"
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/dindel_hmm.h"

namespace dindel {

static const int kAuditMaxRecords = 64;              // differences reported per call; every one is counted

void LikelihoodEngine::setAudit(int windowsPerCall, unsigned long long seed)
{
    audit_ = windowsPerCall > 0 ? windowsPerCall : 0;
    auditSeed_ = seed;
    auditCall_ = &LikelihoodEngine::auditedCall;
}

void LikelihoodEngine::setAuditFaster(int windowsPerCall, unsigned long long seed)
{
    auditFaster_ = windowsPerCall > 0 ? windowsPerCall : 0;
    auditSeed_ = seed;
    auditFasterCall_ = &LikelihoodEngine::auditedFasterCall;
}

const char *LikelihoodEngine::auditFieldName(int field)
{
    static const char *names[DD_AUDIT_N_FIELDS] = {"status", "ll", "llOn", "llOff", "mLogBQ", "offHap", "offHapHMQ", "numIndels", "numMismatch", "nBQT",
                                                   "nmmBQT", "nMMLeft", "nMMRight", "firstBase", "lastBase", "hpos", "var_covered", "var_fcov"};
    return field >= 0 && field < DD_AUDIT_N_FIELDS ? names[field] : "?";
}

// a call's report (the library's bytes) as the engine's: pairs become indices inside their job's window
static void take_report(LikelihoodEngine::AuditReport &A, const std::vector<uint64_t> &report, int n_chosen, const std::vector<int64_t> &full, int W)
{
    dd_audit_report h;
    std::memcpy(&h, report.data(), sizeof(h));
    A.windows = h.n_pairs > 0 ? n_chosen : 0;
    A.pairs = h.n_pairs;
    A.mismatches = h.n_diff;
    const unsigned char *recs = reinterpret_cast<const unsigned char *>(report.data()) + sizeof(h);
    for (long long i = 0; i < h.n_diff && i < kAuditMaxRecords; i++) {
        dd_audit_record r;
        std::memcpy(&r, recs + size_t(i) * sizeof(r), sizeof(r));
        LikelihoodEngine::AuditDifference d;
        d.job = r.window; d.field = r.field;
        d.pair = r.window >= 0 && r.window < W ? r.pair - full[size_t(r.window)] : r.pair;
        d.index = r.index; d.primaryBits = r.primary_bits; d.shadowBits = r.shadow_bits;
        A.differences.push_back(d);
    }
}

// dd_compute_likelihoods_ex with the audit of audit_ windows of this batch behind it; the report of the call becomes auditReport().  The
// sample is a function of the engine's seed and the batch: the seed of a call is the engine's mixed with the batch's first window position.
int LikelihoodEngine::auditedCall(LikelihoodEngine &E, const void *params, const void *batch, void *result, unsigned options)
{
    const dd_params *P = static_cast<const dd_params *>(params);
    const dd_batch *B = static_cast<const dd_batch *>(batch);
    AuditReport &A = E.auditReport_;
    A = AuditReport();
    const int W = B->n_windows;
    const unsigned long long seed = E.auditSeed_ ^ (0x9E3779B97F4A7C15ull * (unsigned long long)(W > 0 ? B->win_hap_start[0] : 0u));
    // the number of windows the library will choose: its own screening and its own choice, repeated here (host arithmetic)
    std::vector<uint8_t> cls(size_t(W) + 1), chosen(size_t(W) + 1);
    std::vector<int64_t> po(size_t(W) + 1), ho(size_t(W) + 1), vo(size_t(W) + 1), full(size_t(W) + 1);
    int32_t mx[4];
    const int bad = options ? dd_screen_windows_ex(P, B, options, cls.data(), mx) : dd_screen_windows(B, cls.data(), mx);
    dd_audit_sizes sz;
    std::memset(&sz, 0, sizeof(sz));
    if (bad < 0 || dd_audit_select(P, B, cls.data(), seed, E.audit_, chosen.data(), po.data(), ho.data(), vo.data(), &sz) < 0) return DD_ERR_INVALID;
    dd_batch_offsets(B, full.data(), NULL, NULL);
    if (E.auditInject_ >= 0 && E.auditInject_ < W) {
        if (chosen[size_t(E.auditInject_)] == DD_WIN_LONG) dd_audit_inject_next(E.auditInject_);    // test hook; a job outside the sample: nothing planted
    }
    E.auditInject_ = -1;
    std::vector<uint64_t> report((DD_AUDIT_REPORT_BYTES(kAuditMaxRecords) + 7) / 8);
    const int rc = dd_compute_likelihoods_audit(P, B, static_cast<dd_result *>(result), E.device_, options, seed, E.audit_, report.data(), kAuditMaxRecords);
    if (rc != DD_SUCCESS) return rc;
    take_report(A, report, sz.n_windows, full, W);
    return DD_SUCCESS;
}

// dd_compute_likelihoods_faster_ex (keys == NULL) or dd_compute_likelihoods_faster_keys with the audit of auditFaster_ windows of this batch
// behind it (dd_compute_likelihoods_faster_audit): the --faster model against its independent shadow kernel.  Seed, report and test hook as
// auditedCall's.
int LikelihoodEngine::auditedFasterCall(LikelihoodEngine &E, const void *params, const void *batch, void *result, short *keys, unsigned options)
{
    const dd_params *P = static_cast<const dd_params *>(params);
    const dd_batch *B = static_cast<const dd_batch *>(batch);
    AuditReport &A = E.auditReport_;
    A = AuditReport();
    const int W = B->n_windows;
    const unsigned long long seed = E.auditSeed_ ^ (0x9E3779B97F4A7C15ull * (unsigned long long)(W > 0 ? B->win_hap_start[0] : 0u));
    std::vector<uint8_t> cls(size_t(W) + 1), chosen(size_t(W) + 1);
    std::vector<int64_t> po(size_t(W) + 1), ho(size_t(W) + 1), vo(size_t(W) + 1), full(size_t(W) + 1);
    int32_t mx[4];
    const int bad = options ? dd_screen_windows_ex(P, B, options, cls.data(), mx) : dd_screen_windows(B, cls.data(), mx);
    dd_audit_sizes sz;
    std::memset(&sz, 0, sizeof(sz));
    if (bad < 0 || dd_audit_select_faster(P, B, cls.data(), options, seed, E.auditFaster_, chosen.data(), po.data(), ho.data(), vo.data(), &sz) < 0)
        return DD_ERR_INVALID;
    dd_batch_offsets(B, full.data(), NULL, NULL);
    if (E.auditInject_ >= 0 && E.auditInject_ < W) {
        if (chosen[size_t(E.auditInject_)] == DD_WIN_LONG) dd_audit_inject_next(E.auditInject_);    // test hook; a job outside the sample: nothing planted
    }
    E.auditInject_ = -1;
    std::vector<uint64_t> report((DD_AUDIT_REPORT_BYTES(kAuditMaxRecords) + 7) / 8);
    const int rc = dd_compute_likelihoods_faster_audit(P, B, static_cast<dd_result *>(result), keys, E.device_, options, seed, E.auditFaster_, report.data(),
                                                       kAuditMaxRecords);
    if (rc != DD_SUCCESS) return rc;
    take_report(A, report, sz.n_windows, full, W);
    return DD_SUCCESS;
}

} // namespace dindel
