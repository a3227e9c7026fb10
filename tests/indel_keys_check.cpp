// indel_keys_check.cpp — the host side of the device indel keys on its own, for a build under AddressSanitizer and UBSan
// (tests/test_indel_keys_cpu.py compiles it with host/compute_likelihoods.cpp and host/device_indel_keys.cpp and runs it as a program; no
// GPU, no HIP).  The C ABI the adapter calls is stubbed here: dd_compute_likelihoods_faster_keys checks what
// LikelihoodEngine::setDeviceIndelKeys asks for (no alignments, the option bits, one int16 per pair) and hands back scripted counts, which
// must come out of the lazy views pair for pair and out of indelCount; a pair scripted as DD_INDEL_KEYS_OVERFLOW makes indelCount
// recompute its window with alignments (the stubbed dd_compute_likelihoods_faster hands back an alignment with 70 distinct keys) once, and
// counts it; a batch with an eager job, and the main model, run as without the switch; and the adapter's own walk over hand-made
// alignments agrees with csrc/indel_keys_kernel.h's.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../dindel_tgi_amd/host/compute_likelihoods.hpp"
#include "../dindel_tgi_amd/csrc/indel_keys_kernel.h"
#include "../include/dindel_hmm.h"

using namespace dindel;

namespace {
int g_failed = 0, g_key_calls = 0, g_faster_calls = 0, g_main_calls = 0;
uint32_t g_expect_options = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); g_failed++; } } while (0)

std::vector<int16_t> g_keys;                          // per pair of the batch: what the stubbed device hands back
const int kManyKeys = 70, kLongRead = 2 * kManyKeys;  // the alignment of every pair with a read that long: 70 distinct keys

void sizes_of(const dd_batch *b, dd_sizes *s, int64_t *po, int64_t *ho, int64_t *vo)
{
    std::memset(s, 0, sizeof(*s));
    for (int w = 0; w < b->n_windows; w++) {
        const int g0 = b->win_hap_off[w], g1 = b->win_hap_off[w + 1], q0 = b->win_read_off[w], q1 = b->win_read_off[w + 1];
        if (po) po[w] = s->n_pairs;
        if (ho) ho[w] = s->hpos_len;
        if (vo) vo[w] = s->var_cov_len;
        s->n_pairs += int64_t(g1 - g0) * (q1 - q0);
        s->hpos_len += int64_t(g1 - g0) * (b->read_seq_off[q1] - b->read_seq_off[q0]);
        s->var_cov_len += int64_t(b->hap_var_off[g1] - b->hap_var_off[g0]) * (q1 - q0);
    }
    if (po) po[b->n_windows] = s->n_pairs;
    if (ho) ho[b->n_windows] = s->hpos_len;
    if (vo) vo[b->n_windows] = s->var_cov_len;
    s->n_haps = b->win_hap_off[b->n_windows]; s->n_reads = b->win_read_off[b->n_windows];
    s->hap_bases = b->hap_seq_off[s->n_haps]; s->read_bases = b->read_seq_off[s->n_reads];
}

// every array the caller asked for, as a device that computed every pair would leave it; hpos: base b of a read is on haplotype base 0
// when b is odd and an inserted base keyed 1000 + b when b is even (a read of 140 bases has 70 distinct keys, a short one few)
void fill_ok(const dd_batch *b, dd_result *r)
{
    dd_sizes s;
    sizes_of(b, &s, NULL, NULL, NULL);
    const size_t np = size_t(s.n_pairs);
    for (size_t p = 0; p < np; p++) {
        r->ll[p] = -1.0 - double(p); r->status[p] = DD_PAIR_OK;
        if (r->llOn) r->llOn[p] = -1.0;
        if (r->llOff) r->llOff[p] = -2.0;
        if (r->mLogBQ) r->mLogBQ[p] = 0.0;
        if (r->offHap) r->offHap[p] = 0;
        if (r->offHapHMQ) r->offHapHMQ[p] = 0;
        int16_t *counters[] = {r->numIndels, r->numMismatch, r->nBQT, r->nmmBQT, r->nMMLeft, r->nMMRight};
        for (size_t i = 0; i < sizeof(counters) / sizeof(*counters); i++) if (counters[i]) counters[i][p] = 0;
        if (r->firstBase) r->firstBase[p] = 0;
        if (r->lastBase) r->lastBase[p] = 0;
    }
    if (r->var_covered) std::memset(r->var_covered, 0, size_t(s.var_cov_len));
    if (r->var_fcov) std::memset(r->var_fcov, 0, size_t(s.var_cov_len));
    if (r->hpos) {
        int64_t at = 0;
        for (int w = 0; w < b->n_windows; w++)
            for (int g = b->win_hap_off[w]; g < b->win_hap_off[w + 1]; g++)
                for (int q = b->win_read_off[w]; q < b->win_read_off[w + 1]; q++) {
                    const int L = b->read_seq_off[q + 1] - b->read_seq_off[q];
                    for (int i = 0; i < L; i++) r->hpos[at++] = int16_t((i & 1) ? 0 : DD_HPOS_INS_KEY0 - (1000 + i));
                }
    }
}
} // namespace

// ---- the C ABI as the adapter sees it ----
extern "C" {
void *dd_host_alloc(size_t) { return NULL; }          // the adapter falls back to malloc: the sanitizer sees every result buffer
void dd_host_free(void *) {}
const char *dd_last_error(void) { return "stub"; }
int dd_reserve_cache(int, size_t, size_t) { return DD_SUCCESS; }
int dd_batch_sizes(const dd_batch *b, dd_sizes *s) { sizes_of(b, s, NULL, NULL, NULL); return DD_SUCCESS; }
int dd_batch_offsets(const dd_batch *b, int64_t *po, int64_t *ho, int64_t *vo) { dd_sizes s; sizes_of(b, &s, po, ho, vo); return DD_SUCCESS; }
int dd_compute_likelihoods(const dd_params *, const dd_batch *b, dd_result *r, int) { g_main_calls++; fill_ok(b, r); return DD_SUCCESS; }
int dd_compute_likelihoods_ex(const dd_params *, const dd_batch *, dd_result *, int, uint32_t) { return DD_ERR_NO_DEVICE; }
int dd_compute_likelihoods_faster(const dd_params *, const dd_batch *b, dd_result *r, int)
{
    g_faster_calls++;
    CHECK(r->hpos != NULL);                           // whoever comes here wants the alignments
    fill_ok(b, r);
    return DD_SUCCESS;
}
int dd_compute_likelihoods_faster_ex(const dd_params *p, const dd_batch *b, dd_result *r, int device, uint32_t options)
{
    CHECK(options == DD_OPT_LONG_WINDOWS_FASTER);
    return dd_compute_likelihoods_faster(p, b, r, device);
}
int dd_compute_likelihoods_cigars(const dd_params *, const dd_batch *, dd_result *, const int32_t *, const uint8_t *, const dd_cigar_result *, int, int, uint32_t)
{
    return DD_ERR_NO_DEVICE;
}
int dd_compute_likelihoods_realign(const dd_params *, const dd_batch *, dd_result *, int, const int32_t *, const int32_t *, const int32_t *, const uint8_t *,
                                   const dd_realign_result *, int, int, uint32_t)
{
    return DD_ERR_NO_DEVICE;
}
int dd_compute_likelihoods_faster_keys(const dd_params *p, const dd_batch *b, dd_result *r, int16_t *keys_out, int device, uint32_t options)
{
    g_key_calls++;
    CHECK(p && p->mapUnmappedReads == 0);
    CHECK(r->hpos == NULL && r->ll != NULL && r->status != NULL && r->onHap == NULL);   // no alignments asked for: the point of the entry
    CHECK(keys_out != NULL && device == 3 && options == g_expect_options);
    dd_sizes s;
    sizes_of(b, &s, NULL, NULL, NULL);
    CHECK(size_t(s.n_pairs) == g_keys.size());
    fill_ok(b, r);
    for (size_t i = 0; i < g_keys.size() && i < size_t(s.n_pairs); i++) keys_out[i] = g_keys[i];
    return DD_SUCCESS;
}
} // extern "C"

namespace {
Read make_read(int L)
{
    Read R;
    R.seq.seq = std::string(size_t(L), 'A');
    R.qual.assign(size_t(L), 0.99);
    R.mapQual = 0.999;
    return R;
}

void test_views_and_fallback(bool long_faster)
{
    ObservationModelParameters prm;
    prm.setCLIDefaultValues();
    LikelihoodEngine eng(prm, 3);
    eng.setDeviceIndelKeys(true);
    eng.setLongWindowsFaster(long_faster);
    eng.setHostThreads(2);
    g_expect_options = long_faster ? DD_OPT_LONG_WINDOWS_FASTER : 0u;
    CHECK(eng.deviceIndelKeys());
    // window 0: 2 haplotypes x 3 reads (5, 70 and 140 bases); window 1: no read; window 2: 1 haplotype x 2 reads
    std::vector<std::vector<Haplotype> > haps(3);
    std::vector<std::vector<Read> > reads(3);
    haps[0].push_back(Haplotype(std::string(40, 'A'))); haps[0].push_back(Haplotype(std::string(41, 'C')));
    reads[0].push_back(make_read(5)); reads[0].push_back(make_read(70)); reads[0].push_back(make_read(kLongRead));
    haps[1].push_back(Haplotype(std::string(30, 'G')));
    haps[2].push_back(Haplotype(std::string(35, 'T')));
    reads[2].push_back(make_read(kLongRead)); reads[2].push_back(make_read(1));
    const int16_t scripted[] = {0, 3, DD_INDEL_KEYS_OVERFLOW, 64, 1, DD_INDEL_KEYS_OVERFLOW, 7, 2};
    g_keys.assign(scripted, scripted + 8);
    std::vector<WindowJob> jobs(3);
    for (size_t w = 0; w < 3; w++) { jobs[w].haps = &haps[w]; jobs[w].reads = &reads[w]; jobs[w].leftPos = uint32_t(100 * (w + 1)); jobs[w].rightPos = jobs[w].leftPos + 50; }
    const int key_calls = g_key_calls, faster_calls = g_faster_calls;
    const long fallbacks = LikelihoodEngine::indelKeyFallbacks();
    eng.computeLikelihoodsFasterBatch(jobs);
    CHECK(g_key_calls == key_calls + 1 && g_faster_calls == faster_calls);
    CHECK(eng.lastHposBytes == 0 && eng.lastIndelKeyBytes == 8 * sizeof(int16_t));
    size_t p = 0;
    for (size_t w = 0; w < 3; w++) {
        CHECK(jobs[w].error.empty() && jobs[w].result.valid() && jobs[w].result.hasDeviceIndelKeys());
        for (size_t h = 0; h < haps[w].size(); h++)
            for (size_t r = 0; r < reads[w].size(); r++, p++) {
                CHECK(jobs[w].result.deviceIndelKeys(h, r) == scripted[p]);
                CHECK(jobs[w].result.ll(h, r) == -1.0 - double(p));
                if (scripted[p] >= 0) CHECK(jobs[w].result.indelCount(h, r) == scripted[p]);
            }
    }
    CHECK(p == 8 && g_faster_calls == faster_calls && LikelihoodEngine::indelKeyFallbacks() == fallbacks);   // nothing recomputed so far
    // the two pairs over the cap: window 0 is recomputed with alignments once, by an engine of the call's own, and both are counted
    CHECK(jobs[0].result.indelCount(0, 2) == kManyKeys);
    CHECK(g_faster_calls == faster_calls + 1 && LikelihoodEngine::indelKeyFallbacks() == fallbacks + 1);
    CHECK(jobs[0].result.indelCount(1, 2) == kManyKeys);
    CHECK(g_faster_calls == faster_calls + 1 && LikelihoodEngine::indelKeyFallbacks() == fallbacks + 2);
    CHECK(eng.deviceIndelKeys() && g_key_calls == key_calls + 1);
    // get() on such a view: the existing recompute path of the engine, which asks for alignments and comes back with the switch still on
    const MLAlignment ml = jobs[2].result.get(0, 0);
    CHECK(int(ml.indels.size()) == kManyKeys && g_faster_calls == faster_calls + 2 && eng.deviceIndelKeys());

    // a batch with an eager job runs as without the switch: alignments, no keys
    std::vector<std::vector<MLAlignment> > liks;
    std::vector<int> onHap;
    jobs[2].liks = &liks; jobs[2].onHap = &onHap;
    eng.computeLikelihoodsFasterBatch(jobs);
    CHECK(g_key_calls == key_calls + 1 && g_faster_calls == faster_calls + 3);
    CHECK(!jobs[0].result.hasDeviceIndelKeys() && eng.lastIndelKeyBytes == 0 && eng.lastHposBytes > 0);
    CHECK(jobs[0].result.indelCount(0, 1) == 35 && jobs[0].result.indelCount(0, 2) == kManyKeys);            // the adapter's own walk
    CHECK(liks.size() == 1 && liks[0].size() == 2 && int(liks[0][0].indels.size()) == kManyKeys);
    jobs[2].liks = NULL; jobs[2].onHap = NULL;

    // the main model does not know the switch
    const int main_calls = g_main_calls;
    eng.computeLikelihoodsBatch(jobs);
    CHECK(g_main_calls == main_calls + 1 && g_key_calls == key_calls + 1 && !jobs[0].result.hasDeviceIndelKeys());
}

void test_walk_agrees_with_the_shared_header()
{
    const int16_t I = DD_HPOS_INS, LO = DD_HPOS_LO, RO = DD_HPOS_RO;
    const int16_t K5 = int16_t(DD_HPOS_INS_KEY0 - 5);
    const int16_t a0[] = {I, I, 4, 5, 9, K5, I, 10, LO, 12, 20, RO, I};
    const int16_t a1[] = {7, 3, 32767, 0, -32768, -17, 5, -2, 8};
    const int16_t a2[] = {K5, 1, K5, 4, I};
    const int16_t *arrays[] = {a0, a1, a2};
    const int lens[] = {13, 9, 5};
    const int want[] = {5, 2, 1};
    for (int i = 0; i < 3; i++) {
        std::vector<Haplotype> haps(1, Haplotype(std::string(32768, 'A')));
        std::vector<Read> reads(1, make_read(lens[i]));
        const WindowLikelihoods v = WindowLikelihoods::handMadeFaster(haps, reads, arrays[i], NULL);
        CHECK(v.indelCount(0, 0) == ik_count_serial(arrays[i], lens[i]));
        CHECK(v.indelCount(0, 0) == want[i]);
        const int16_t key = 9;
        const WindowLikelihoods k = WindowLikelihoods::handMadeFaster(haps, reads, NULL, &key);
        CHECK(k.hasDeviceIndelKeys() && k.indelCount(0, 0) == 9);
    }
}
} // namespace

int main()
{
    try {
        test_views_and_fallback(false);
        test_views_and_fallback(true);
        test_walk_agrees_with_the_shared_header();
    } catch (std::string &e) {
        std::printf("FAILED: threw %s\n", e.c_str());
        return 1;
    }
    if (g_failed) { std::printf("indel_keys_check: %d check(s) failed\n", g_failed); return 1; }
    std::printf("indel_keys_check: ok\n");
    return 0;
}
