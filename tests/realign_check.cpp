// realign_check.cpp — the host side of the device realign on its own, for a build under AddressSanitizer and UBSan (tests/test_realign_cpu.py
// compiles it with host/compute_likelihoods.cpp, host/realigned_bam.cpp and the units they stand on, and runs it as a program; no GPU, no
// HIP).  The C ABI the adapter calls is stubbed here: dd_compute_likelihoods_realign checks what LikelihoodEngine::setDeviceRealign packs
// (mode, onHap asked for, no alignments asked for, every haplotype's refHpos and aligned flag at its offset) and hands back scripted rows,
// which must then come out of the lazy views read for read; pooledRealignedCigars consumes those views — DD_REALIGN_OFF_HAP, windows
// without haplotypes or reads, every throw code, operation rows at the cap, and reads over the cap with and without alignments at hand.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>
#include "../dindel_tgi_amd/host/cigar.hpp"
#include "../dindel_tgi_amd/host/compute_likelihoods.hpp"
#include "../dindel_tgi_amd/host/realigned_bam.hpp"
#include "../include/dindel_hmm.h"

using namespace dindel;

namespace {
int g_failed = 0, g_calls = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); g_failed++; } } while (0)

const int kCap = 2;
std::vector<std::vector<Haplotype> > g_haps;          // per window
std::vector<std::vector<Read> > g_reads;
struct Row { int hap, status, n_ops, ref_off; uint32_t ops[kCap]; };
std::vector<Row> g_rows;                              // per read of the batch: what the stubbed device hands back

void sizes_of(const dd_batch *b, dd_sizes *s, int64_t *po, int64_t *ho, int64_t *vo)
{
    std::memset(s, 0, sizeof(*s));
    for (int w = 0; w < b->n_windows; w++) {
        const int g0 = b->win_hap_off[w], g1 = b->win_hap_off[w + 1], q0 = b->win_read_off[w], q1 = b->win_read_off[w + 1];
        if (po) { po[w] = s->n_pairs; ho[w] = s->hpos_len; vo[w] = s->var_cov_len; }
        s->n_pairs += int64_t(g1 - g0) * (q1 - q0);
        s->hpos_len += int64_t(g1 - g0) * (b->read_seq_off[q1] - b->read_seq_off[q0]);
        s->var_cov_len += int64_t(b->hap_var_off[g1] - b->hap_var_off[g0]) * (q1 - q0);
    }
    if (po) { po[b->n_windows] = s->n_pairs; ho[b->n_windows] = s->hpos_len; vo[b->n_windows] = s->var_cov_len; }
    s->n_haps = b->win_hap_off[b->n_windows]; s->n_reads = b->win_read_off[b->n_windows];
    s->hap_bases = b->hap_seq_off[s->n_haps]; s->read_bases = b->read_seq_off[s->n_reads];
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
int dd_compute_likelihoods(const dd_params *, const dd_batch *, dd_result *, int) { return DD_ERR_NO_DEVICE; }
int dd_compute_likelihoods_ex(const dd_params *, const dd_batch *, dd_result *, int, uint32_t) { return DD_ERR_NO_DEVICE; }
int dd_compute_likelihoods_faster(const dd_params *, const dd_batch *, dd_result *, int) { return DD_ERR_NO_DEVICE; }
int dd_compute_likelihoods_faster_ex(const dd_params *, const dd_batch *, dd_result *, int, uint32_t) { return DD_ERR_NO_DEVICE; }
int dd_compute_likelihoods_cigars(const dd_params *, const dd_batch *, dd_result *, const int32_t *, const uint8_t *, const dd_cigar_result *, int, int, uint32_t)
{
    return DD_ERR_NO_DEVICE;
}
int dd_compute_likelihoods_realign(const dd_params *, const dd_batch *b, dd_result *r, int mode, const int32_t *win_hap_pair, const int32_t *hap_n_indels,
                                   const int32_t *hap_ref_pos, const uint8_t *hap_aligned, const dd_realign_result *out, int ops_cap, int, uint32_t options)
{
    g_calls++;
    CHECK(mode == DD_REALIGN_FIRST_MAX && !win_hap_pair && !hap_n_indels && options == 0 && ops_cap == kCap);
    CHECK(r->onHap != NULL && r->hpos == NULL && r->ll != NULL && r->status != NULL);
    CHECK(out && out->hap && out->status && out->n_ops && out->ops && out->ref_off);
    CHECK(b->n_windows == int(g_haps.size()));
    dd_sizes s;
    sizes_of(b, &s, NULL, NULL, NULL);
    for (int w = 0; w < b->n_windows; w++) {                                 // the packing: refHpos and the aligned flag of every haplotype
        CHECK(b->win_hap_off[w + 1] - b->win_hap_off[w] == int(g_haps[size_t(w)].size()));
        for (size_t h = 0; h < g_haps[size_t(w)].size(); h++) {
            const Haplotype &H = g_haps[size_t(w)][h];
            const int g = b->win_hap_off[w] + int(h);
            const bool aligned = H.refHpos.size() == H.seq.size();
            CHECK(b->hap_seq_off[g + 1] - b->hap_seq_off[g] == int(H.seq.size()));
            CHECK(hap_aligned[g] == (aligned ? 1 : 0));
            for (size_t i = 0; i < H.seq.size(); i++) CHECK(hap_ref_pos[size_t(b->hap_seq_off[g]) + i] == (aligned ? H.refHpos[i] : 0));
        }
    }
    for (int64_t p = 0; p < s.n_pairs; p++) { r->ll[p] = -1.0 - double(p); r->status[p] = DD_PAIR_OK; r->offHapHMQ[p] = 0; }
    CHECK(size_t(s.n_reads) == g_rows.size());
    for (int64_t q = 0; q < s.n_reads; q++) {
        const Row &R = g_rows[size_t(q)];
        r->onHap[q] = R.status != DD_REALIGN_OFF_HAP;
        out->hap[q] = R.hap; out->status[q] = R.status; out->n_ops[q] = R.n_ops; out->ref_off[q] = R.ref_off;
        for (int i = 0; i < kCap; i++) out->ops[q * kCap + i] = R.ops[i];
    }
    return DD_SUCCESS;
}
}

namespace {

Haplotype hap_at(int len, int shift, bool aligned)
{
    Haplotype H(std::string(size_t(len), 'C'));
    if (aligned) for (int i = 0; i < len; i++) H.refHpos.push_back(shift + i);
    return H;
}

Read read_of(int len)
{
    Read R;
    R.seq = Haplotype(std::string(size_t(len), 'C'));
    R.setAllQual(0.999);
    R.mapQual = 0.9999;
    return R;
}

uint32_t word(int op, int len) { return (uint32_t(len) << 4) | uint32_t(op); }

// hand-made alignments of a window: read r lies on haplotype h from base h + r on, with one deleted haplotype base in its middle when
// `gap` (M D M: three operations, over the cap of two)
std::vector<int16_t> hpos_of(const std::vector<Haplotype> &haps, const std::vector<Read> &reads, bool gap)
{
    std::vector<int16_t> v;
    for (size_t h = 0; h < haps.size(); h++)
        for (size_t r = 0; r < reads.size(); r++)
            for (size_t b = 0; b < reads[r].size(); b++) v.push_back(int16_t(h + r + b + (gap && b >= reads[r].size() / 2 ? 1 : 0)));
    return v;
}

std::string thrown_by(const std::vector<Haplotype> &haps, const std::vector<Read> &reads, const WindowLikelihoods &v, const std::function<WindowLikelihoods()> &wa)
{
    std::vector<CIGAR> c;
    long fb = 0;
    try { pooledRealignedCigars(haps, reads, v, 1000, c, wa, &fb); } catch (const std::string &e) { return e; }
    return "";
}

} // namespace

int main()
{
    // ---- three windows through the engine: one ordinary, one without haplotypes, one without reads, one more ordinary ----
    g_haps.resize(4); g_reads.resize(4);
    g_haps[0].push_back(hap_at(60, 0, true)); g_haps[0].push_back(hap_at(61, 10, true)); g_haps[0].push_back(hap_at(40, 0, false));
    for (int r = 0; r < 5; r++) g_reads[0].push_back(read_of(20 + r));
    for (int r = 0; r < 2; r++) g_reads[1].push_back(read_of(30));           // window 1: reads, no haplotype
    g_haps[2].push_back(hap_at(50, 5, true));                                // window 2: a haplotype, no read
    g_haps[3].push_back(hap_at(70, 3, true)); g_haps[3].push_back(hap_at(70, 4, true));
    for (int r = 0; r < 3; r++) g_reads[3].push_back(read_of(36));
    const Row rows[] = {
        {1, DD_CIGAR_OK, 1, 11, {word(0, 20), 0}}, {-1, DD_REALIGN_OFF_HAP, 0, -1, {0, 0}}, {0, DD_CIGAR_OK, 2, 2, {word(4, 3), word(0, 19)}},
        {1, DD_CIGAR_OVERFLOW, 3, 14, {word(0, 11), word(2, 1)}}, {0, DD_CIGAR_OK, 1, -1, {word(4, 24), 0}},
        {-1, DD_REALIGN_NO_HAPS, 0, -1, {0, 0}}, {-1, DD_REALIGN_NO_HAPS, 0, -1, {0, 0}},
        {1, DD_CIGAR_OK, 1, 4, {word(0, 36), 0}}, {0, DD_CIGAR_NOT_COMPUTED, 0, -1, {0, 0}}, {1, DD_CIGAR_OVERFLOW, 3, 6, {word(0, 18), word(2, 1)}},
    };
    g_rows.assign(rows, rows + sizeof(rows) / sizeof(rows[0]));
    ObservationModelParameters obs;
    obs.setCLIDefaultValues();
    LikelihoodEngine engine(obs);
    engine.setKeepAlignments(false);
    engine.setDeviceCigars(true, 5);                                         // device realign wins over it, cap included
    engine.setDeviceRealign(true, kCap);
    std::vector<WindowJob> jobs(4);
    for (size_t w = 0; w < 4; w++) { jobs[w].haps = &g_haps[w]; jobs[w].reads = &g_reads[w]; jobs[w].leftPos = uint32_t(1000 + 100 * w); jobs[w].rightPos = jobs[w].leftPos + 50; }
    engine.computeLikelihoodsBatch(jobs);
    CHECK(g_calls == 1);
    CHECK(engine.lastRealignBytes == g_rows.size() * (16 + 4 * kCap) && engine.lastHposBytes == 0 && engine.lastCigarBytes == 0);
    size_t q = 0;
    for (size_t w = 0; w < 4; w++) {
        const WindowLikelihoods &v = jobs[w].result;
        CHECK(jobs[w].error.empty() && v.valid() && v.hasDeviceRealign() && !v.hasDeviceCigars() && v.cigarOpsCap() == kCap);
        for (size_t r = 0; r < g_reads[w].size(); r++, q++) {
            const Row &R = g_rows[q];
            CHECK(v.realignHap(r) == R.hap && v.realignStatus(r) == R.status && v.realignNumOps(r) == R.n_ops && v.realignRefOff(r) == R.ref_off);
            CHECK(std::memcmp(v.realignOps(r), R.ops, sizeof(R.ops)) == 0);
        }
    }
    CHECK(q == g_rows.size());

    // ---- the consumer on those views ----
    for (size_t w = 0; w < 4; w++) {
        const std::vector<Haplotype> &haps = g_haps[w];
        const std::vector<Read> &reads = g_reads[w];
        const std::vector<int16_t> hp = hpos_of(haps, reads, true);
        int made = 0;
        const std::function<WindowLikelihoods()> wa = [&]() { made++; return WindowLikelihoods::handMadeRealign(haps, reads, kCap, NULL, NULL, NULL, NULL, NULL, hp.data()); };
        std::vector<CIGAR> cigars;
        long fb = 0;
        pooledRealignedCigars(haps, reads, jobs[w].result, 1000, cigars, wa, &fb);
        CHECK(cigars.size() == reads.size());
        if (w == 0) {
            CHECK(fb == 1 && made == 1);
            CHECK(cigars[0].size() == 1 && cigars[0][0].first == 0 && cigars[0][0].second == 20 && cigars[0].refPos == 1011);
            CHECK(cigars[1].empty() && cigars[1].refPos == -1);                            // DD_REALIGN_OFF_HAP
            CHECK(cigars[2].size() == 2 && cigars[2][0].first == 4 && cigars[2][1].second == 19 && cigars[2].refPos == 1002);
            MLAlignment ml;                                                                // the read over the cap: getCIGAR on haplotype 1
            for (size_t b = 0; b < reads[3].size(); b++) ml.hpos.push_back(int(1 + 3 + b + (b >= reads[3].size() / 2 ? 1 : 0)));
            const CIGAR want = getCIGAR(haps[1].refHpos, haps[1].size(), ml, reads[3].size(), 1000);
            CHECK(want.size() == 3 && cigars[3].size() == 3 && cigars[3].refPos == want.refPos);
            for (size_t i = 0; i < 3 && i < cigars[3].size(); i++) CHECK(cigars[3][i] == want[i]);
            CHECK(cigars[4].size() == 1 && cigars[4].refPos == -1);                        // nothing aligned: refPos stays -1
        } else if (w == 1) {
            CHECK(fb == 0 && made == 0 && cigars[0].empty() && cigars[1].empty());         // no haplotypes: no read is on one
        } else if (w == 2) {
            CHECK(fb == 0 && cigars.empty());
        } else {
            CHECK(fb == 2 && made == 1);                                                   // DD_CIGAR_NOT_COMPUTED and DD_CIGAR_OVERFLOW share the window's alignments
            CHECK(cigars[1].size() == 3 && cigars[2].size() == 3 && cigars[1].refPos == 1000 + 3 + 1 && cigars[2].refPos == 1000 + 4 + 1 + 2);
        }
    }
    // a read over the cap and nothing at hand
    CHECK(thrown_by(g_haps[0], g_reads[0], jobs[0].result, std::function<WindowLikelihoods()>()) == "realignedCigars: a read needs the host getCIGAR and no alignments are at hand");

    // ---- hand-made views: every throw code raises getCIGAR's string, at the first read that has one ----
    const char *const msg[] = {"", "Haplotype has not been aligned!", "Error(1)!", "Error(2)!", "Error(3)!", "Error(4)!", "How is this possible? (1)"};
    const std::vector<Haplotype> &haps = g_haps[0];
    const std::vector<Read> &reads = g_reads[0];
    for (int code = DD_CIGAR_HAP_NOT_ALIGNED; code <= DD_CIGAR_IMPOSSIBLE; code++) {
        int32_t hap[5] = {0, 1, 2, 0, 1}, status[5] = {DD_CIGAR_OK, DD_REALIGN_OFF_HAP, code, DD_CIGAR_ERROR1, DD_CIGAR_OK}, n_ops[5] = {1, 0, 0, 0, 1}, ref_off[5] = {0, -1, -1, -1, 0};
        uint32_t ops[5 * kCap] = {word(0, 20), 0, 0, 0, 0, 0, 0, 0, word(0, 24), 0};
        const WindowLikelihoods v = WindowLikelihoods::handMadeRealign(haps, reads, kCap, hap, status, n_ops, ops, ref_off, NULL);
        CHECK(thrown_by(haps, reads, v, std::function<WindowLikelihoods()>()) == msg[code]);
    }
    {   // a row that names no haplotype of the window is refused, not indexed
        int32_t hap[5] = {0, 0, 3, 0, 0}, status[5] = {0, 0, 0, 0, 0}, n_ops[5] = {1, 1, 1, 1, 1}, ref_off[5] = {0, 0, 0, 0, 0};
        uint32_t ops[5 * kCap] = {word(0, 20), 0, word(0, 21), 0, word(0, 22), 0, word(0, 23), 0, word(0, 24), 0};
        const WindowLikelihoods v = WindowLikelihoods::handMadeRealign(haps, reads, kCap, hap, status, n_ops, ops, ref_off, NULL);
        CHECK(thrown_by(haps, reads, v, std::function<WindowLikelihoods()>()) == "pooledDeviceRealignedCigars: no haplotype was chosen for a read");
        status[2] = DD_REALIGN_BAD_PAIR; hap[2] = -1;
        const WindowLikelihoods v2 = WindowLikelihoods::handMadeRealign(haps, reads, kCap, hap, status, n_ops, ops, ref_off, NULL);
        CHECK(thrown_by(haps, reads, v2, std::function<WindowLikelihoods()>()) == "pooledDeviceRealignedCigars: no haplotype was chosen for a read");
    }
    {   // a view without realigned reads goes the old way: the host rule on ll (all 0.0: haplotype 0) over the hand-made alignments
        const std::vector<int16_t> hp = hpos_of(haps, reads, false);
        const WindowLikelihoods v = WindowLikelihoods::handMadeRealign(haps, reads, kCap, NULL, NULL, NULL, NULL, NULL, hp.data());
        std::vector<CIGAR> cigars;
        long fb = 0;
        CHECK(!v.hasDeviceRealign());
        pooledRealignedCigars(haps, reads, v, 1000, cigars, std::function<WindowLikelihoods()>(), &fb);
        CHECK(fb == 0 && cigars.size() == 5 && cigars[2].size() == 1 && cigars[2].refPos == 1002);
    }
    if (g_failed) { std::printf("realign_check: %d checks failed\n", g_failed); return 1; }
    std::printf("realign_check: ok\n");
    return 0;
}
