// diploid_pair_check.cpp — the CPU evaluation of the certified MAP haplotype pair (csrc/diploid_pair_host.cpp) as a program of its own, built by
// tests/test_diploid_pair_cpu.py with g++ alone under AddressSanitizer and UBSan: every array is a heap allocation of exactly its size, so a
// read or write past a window's share is seen.  It checks the states and values that can be worked out by hand and that threads change nothing.
// Then the host side of --deviceRealignDiploid with the C ABI stubbed here (no GPU, no HIP): dd_compute_likelihoods_realign_diploid checks what
// LikelihoodEngine::setDeviceRealignDiploid packs (every window's prior table at its offset, countIndels and refHpos per haplotype, no
// alignments and no onHap asked for), takes the windows' pairs from the real CPU evaluation on scripted likelihoods and hands back scripted
// rows; these must come out of the views, and diploidDeviceRealignedCigars consumes them: certified rows as they are, a read over the cap
// redone on the host, an uncertified window through maxLikelihoodPair and the host's CIGARs.
#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include "../dindel_tgi_amd/host/cigar.hpp"
#include "../dindel_tgi_amd/host/compute_likelihoods.hpp"
#include "../dindel_tgi_amd/host/realigned_bam.hpp"
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>
#include "../include/dindel_hmm.h"

static bool near(double a, double b) { return std::fabs(a - b) < 1e-12; }
#define CHECK(c) do { if (!(c)) { printf("diploid_pair_check: line %d: %s\n", __LINE__, #c); return 1; } } while (0)

namespace {
struct Batch {
    std::vector<int32_t> ho{0}, ro{0}, status;
    std::vector<double> ll, prior;
    void add(int H, int R, const std::vector<double> &l, const std::vector<double> &p, const std::vector<int32_t> &st = std::vector<int32_t>())
    {
        ho.push_back(ho.back() + H); ro.push_back(ro.back() + R);
        ll.insert(ll.end(), l.begin(), l.end()); prior.insert(prior.end(), p.begin(), p.end());
        std::vector<int32_t> s = st.empty() ? std::vector<int32_t>(l.size(), 0) : st;
        status.insert(status.end(), s.begin(), s.end());
    }
};
struct Out {
    std::vector<int32_t> pair, state;
    std::vector<double> best, gap, margin;
    dd_diploid_pair_result r;
    explicit Out(size_t W) : pair(2 * W, 77), state(W, 77), best(W, 77.0), gap(W, 77.0), margin(W, 77.0)
    {
        r.pair = pair.data(); r.state = state.data(); r.best = best.data(); r.gap = gap.data(); r.margin = margin.data();
    }
};
int run(const Batch &b, Out &o, int threads, bool with_status = true)
{
    dd_batch db = dd_batch();
    db.n_windows = int(b.ho.size()) - 1; db.win_hap_off = b.ho.data(); db.win_read_off = b.ro.data();
    return dd_diploid_pairs_host(&db, b.ll.empty() ? NULL : b.ll.data(), with_status ? b.status.data() : NULL, b.prior.empty() ? NULL : b.prior.data(),
                                 &o.r, threads);
}
}

// ---------------------------------------------------------------- the adapter against a stubbed C ABI
using namespace dindel;
namespace {
const int kCap = 2;
int g_calls = 0, g_stub_failed = 0;
#define SCHECK(c) do { if (!(c)) { printf("diploid_pair_check: line %d: %s\n", __LINE__, #c); g_stub_failed++; } } while (0)
std::vector<std::vector<Haplotype> > g_haps;
std::vector<std::vector<Read> > g_reads;
std::vector<std::vector<double> > g_prior;
std::vector<double> g_ll;                              // per pair of the batch
struct Row { int hap, status, n_ops, ref_off; uint32_t ops[kCap]; };
std::vector<Row> g_rows;                               // per read of the batch
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
Haplotype hap_at(int len, int shift, int indels)
{
    Haplotype H(std::string(size_t(len), 'C'));
    for (int i = 0; i < len; i++) H.refHpos.push_back(shift + i);
    for (int i = 0; i < indels; i++) H.indels[10 + i] = AlignedVariant("-A", 10 + i, 10 + i, 10 + i, 10 + i);
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
std::vector<int16_t> hpos_of(const std::vector<Haplotype> &haps, const std::vector<Read> &reads)     // read r on haplotype h from base h + r on, one base deleted in its middle
{
    std::vector<int16_t> v;
    for (size_t h = 0; h < haps.size(); h++)
        for (size_t r = 0; r < reads.size(); r++)
            for (size_t b = 0; b < reads[r].size(); b++) v.push_back(int16_t(h + r + b + (b >= reads[r].size() / 2 ? 1 : 0)));
    return v;
}
}

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
int dd_compute_likelihoods_realign(const dd_params *, const dd_batch *, dd_result *, int, const int32_t *, const int32_t *, const int32_t *, const uint8_t *,
                                   const dd_realign_result *, int, int, uint32_t)
{
    return DD_ERR_NO_DEVICE;
}
int dd_compute_likelihoods_realign_diploid(const dd_params *, const dd_batch *b, dd_result *r, const double *prior, const int32_t *hap_n_indels,
                                           const int32_t *hap_ref_pos, const uint8_t *hap_aligned, const dd_diploid_pair_result *pair_out,
                                           const dd_realign_result *out, int ops_cap, int, uint32_t options)
{
    g_calls++;
    SCHECK(options == 0 && ops_cap == kCap && prior && hap_n_indels && hap_ref_pos && hap_aligned);
    SCHECK(r->onHap == NULL && r->hpos == NULL && r->ll != NULL && r->status != NULL);
    SCHECK(out && out->hap && out->status && out->n_ops && out->ops && out->ref_off);
    SCHECK(pair_out && pair_out->pair && pair_out->state && pair_out->best && pair_out->gap && pair_out->margin);
    SCHECK(b->n_windows == int(g_haps.size()));
    dd_sizes s;
    sizes_of(b, &s, NULL, NULL, NULL);
    size_t hh = 0;
    for (int w = 0; w < b->n_windows; w++) {             // the packing: the prior table, the indel count, refHpos and the aligned flag
        const size_t H = g_haps[size_t(w)].size();
        SCHECK(b->win_hap_off[w + 1] - b->win_hap_off[w] == int(H));
        for (size_t i = 0; i < H * H; i++) SCHECK(prior[hh + i] == g_prior[size_t(w)][i]);
        hh += H * H;
        for (size_t h = 0; h < H; h++) {
            const Haplotype &Hp = g_haps[size_t(w)][h];
            const int g = b->win_hap_off[w] + int(h);
            SCHECK(hap_n_indels[g] == Hp.countIndels() && hap_aligned[g] == 1);
            for (size_t i = 0; i < Hp.seq.size(); i++) SCHECK(hap_ref_pos[size_t(b->hap_seq_off[g]) + i] == Hp.refHpos[i]);
        }
    }
    SCHECK(size_t(s.n_pairs) == g_ll.size() && size_t(s.n_reads) == g_rows.size());
    for (int64_t p = 0; p < s.n_pairs; p++) { r->ll[p] = g_ll[size_t(p)]; r->status[p] = DD_PAIR_OK; r->offHapHMQ[p] = 0; }
    SCHECK(dd_diploid_pairs_host(b, r->ll, r->status, prior, pair_out, 2) == DD_SUCCESS);      // the windows' pairs: the real CPU evaluation
    for (int64_t q = 0; q < s.n_reads; q++) {
        const Row &R = g_rows[size_t(q)];
        out->hap[q] = R.hap; out->status[q] = R.status; out->n_ops[q] = R.n_ops; out->ref_off[q] = R.ref_off;
        for (int i = 0; i < kCap; i++) out->ops[q * kCap + i] = R.ops[i];
    }
    return DD_SUCCESS;
}
}

static int adapter_checks()
{
    // window 0: two haplotypes, the pair (1, 1) far ahead; window 1: reads, no haplotype; window 2: two haplotypes with the same likelihoods
    // and priors (a tie: the host's window); window 3: a haplotype, no read
    g_haps.resize(4); g_reads.resize(4); g_prior.resize(4);
    g_haps[0].push_back(hap_at(60, 0, 0)); g_haps[0].push_back(hap_at(61, 10, 2));
    for (int r = 0; r < 3; r++) g_reads[0].push_back(read_of(20 + r));
    g_prior[0] = {-3.0, -2.0, 0.0, -1.0};
    for (int r = 0; r < 2; r++) g_reads[1].push_back(read_of(30));
    g_haps[2].push_back(hap_at(70, 3, 1)); g_haps[2].push_back(hap_at(70, 3, 1));
    for (int r = 0; r < 2; r++) g_reads[2].push_back(read_of(36));
    g_prior[2] = {-2.5, -2.5, 0.0, -2.5};
    g_haps[3].push_back(hap_at(50, 5, 0));
    g_prior[3] = {-0.75};
    g_ll = {-20.0, -21.0, -22.0, -2.0, -3.0, -2.5, /* window 2 */ -4.0, -5.0, -4.0, -5.0};
    const Row rows[] = {
        {1, DD_CIGAR_OK, 1, 11, {word(0, 20), 0}}, {1, DD_CIGAR_OVERFLOW, 3, 14, {word(0, 10), word(2, 1)}}, {1, DD_CIGAR_OK, 2, 2, {word(4, 3), word(0, 19)}},
        {-1, DD_REALIGN_NO_HAPS, 0, -1, {0, 0}}, {-1, DD_REALIGN_NO_HAPS, 0, -1, {0, 0}},
        {-1, DD_REALIGN_BAD_PAIR, 0, -1, {0, 0}}, {-1, DD_REALIGN_BAD_PAIR, 0, -1, {0, 0}},
    };
    g_rows.assign(rows, rows + sizeof(rows) / sizeof(rows[0]));
    ObservationModelParameters obs;
    obs.setCLIDefaultValues();
    LikelihoodEngine engine(obs);
    engine.setKeepAlignments(false);
    engine.setDeviceCigars(true, 5);                                         // the diploid switch wins over both, cap included
    engine.setDeviceRealign(true, 7);
    engine.setDeviceRealignDiploid(true, kCap);
    std::vector<WindowJob> jobs(4);
    for (size_t w = 0; w < 4; w++) {
        jobs[w].haps = &g_haps[w]; jobs[w].reads = &g_reads[w]; jobs[w].leftPos = uint32_t(1000 + 100 * w); jobs[w].rightPos = jobs[w].leftPos + 50;
        jobs[w].pairPrior = &g_prior[w];
    }
    engine.computeLikelihoodsBatch(jobs);
    SCHECK(g_calls == 1);
    SCHECK(engine.lastRealignBytes == g_rows.size() * (16 + 4 * kCap) + 4 * 36 && engine.lastHposBytes == 0 && engine.lastCigarBytes == 0);
    const int want_state[4] = {DD_DIPPAIR_CERTIFIED, DD_DIPPAIR_NO_HAPS, DD_DIPPAIR_TIE, DD_DIPPAIR_CERTIFIED};
    size_t q = 0;
    for (size_t w = 0; w < 4; w++) {
        const WindowLikelihoods &v = jobs[w].result;
        SCHECK(jobs[w].error.empty() && v.valid() && v.hasDevicePair() && v.hasDeviceRealign() && !v.hasDeviceCigars() && v.cigarOpsCap() == kCap);
        SCHECK(v.pairState() == want_state[w]);
        SCHECK(v.devicePair() == (w == 0 ? std::pair<int, int>(1, 1) : w == 3 ? std::pair<int, int>(0, 0) : std::pair<int, int>(-1, -1)));
        for (size_t r = 0; r < g_reads[w].size(); r++, q++) {
            const Row &R = g_rows[q];
            SCHECK(v.realignHap(r) == R.hap && v.realignStatus(r) == R.status && v.realignNumOps(r) == R.n_ops && v.realignRefOff(r) == R.ref_off);
            SCHECK(std::memcmp(v.realignOps(r), R.ops, sizeof(R.ops)) == 0);
        }
    }
    SCHECK(q == g_rows.size());
    jobs[2].pairPrior = NULL;                                                // a job without its table is refused before anything is packed for the device
    bool refused = false;
    try { engine.computeLikelihoodsBatch(jobs); } catch (const std::string &e) { refused = e.find("pair prior") != std::string::npos; }
    SCHECK(refused && g_calls == 1);

    // ---- the consumer on the first call's views (kept alive by their own references to the block) ----
    jobs[2].pairPrior = &g_prior[2];
    engine.computeLikelihoodsBatch(jobs);
    SCHECK(g_calls == 2);
    const DiploidParameters dip;
    const AlignedCandidates none;
    for (size_t w = 0; w < 4; w++) {
        if (w == 1) continue;                                               // no haplotype: maxLikelihoodPair throws, as without the switch
        const std::vector<Haplotype> &haps = g_haps[w];
        const std::vector<Read> &reads = g_reads[w];
        const std::vector<int16_t> hp = hpos_of(haps, reads);
        int made = 0;
        const std::function<WindowLikelihoods()> wa = [&]() {
            made++;
            return WindowLikelihoods::handMadeRealign(haps, reads, kCap, NULL, NULL, NULL, NULL, NULL, hp.data(), g_ll.data() + (w == 2 ? 6 : 0));
        };
        std::vector<CIGAR> cigars;
        long fb = 0, un = 0;
        const std::pair<int, int> used = diploidDeviceRealignedCigars(haps, reads, jobs[w].result, 0, none, dip, 1000, cigars, wa, &fb, &un);
        SCHECK(cigars.size() == reads.size());
        if (w == 0) {
            SCHECK(used == std::make_pair(1, 1) && un == 0 && fb == 1 && made == 1);
            SCHECK(cigars[0].size() == 1 && cigars[0][0].second == 20 && cigars[0].refPos == 1011);
            SCHECK(cigars[2].size() == 2 && cigars[2][0].first == 4 && cigars[2].refPos == 1002);
            MLAlignment ml;                                                  // the read over the cap: getCIGAR on haplotype 1
            for (size_t b = 0; b < reads[1].size(); b++) ml.hpos.push_back(int(1 + 1 + b + (b >= reads[1].size() / 2 ? 1 : 0)));
            const CIGAR want = getCIGAR(haps[1].refHpos, haps[1].size(), ml, reads[1].size(), 1000);
            SCHECK(want.size() == 3 && cigars[1].size() == 3 && cigars[1].refPos == want.refPos);
        } else if (w == 2) {
            SCHECK(un == 1 && fb == 0 && made == 1 && used.first >= 0 && used.second >= used.first);
            const std::pair<int, int> host = maxLikelihoodPair(haps, reads, jobs[w].result, 0, none, dip);
            SCHECK(used == host && cigars[0].size() == 3 && cigars[1].size() == 3);
        } else {
            SCHECK(used == std::make_pair(0, 0) && un == 0 && fb == 0 && made == 0 && cigars.empty());
        }
    }
    bool thrown = false;                                                     // window 1 throws what the host path throws there
    try {
        std::vector<CIGAR> cigars; long fb = 0, un = 0;
        diploidDeviceRealignedCigars(g_haps[1], g_reads[1], jobs[1].result, 0, none, dip, 1000, cigars, std::function<WindowLikelihoods()>(), &fb, &un);
    } catch (const std::string &e) { thrown = e == "no haplotype pair with a finite likelihood"; }
    SCHECK(thrown);
    return g_stub_failed;
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    Batch b;
    b.add(0, 0, {}, {});                                                          // 0 empty
    b.add(2, 3, {-1, -2, -3, -1.5, -2, -2.5}, {-1, -2, 0, -1.5});                 // 1 certified: (0, 0) = -6 - 1 exactly (ll + log 2 + log .5)
    b.add(0, 4, {}, {});                                                          // 2 reads, no haplotype
    b.add(2, 2, {-3, -4, -3, -4}, {-2, -2, 0, -2});                               // 3 identical columns, equal priors: a tie with gap 0
    b.add(1, 2, {-5, -6}, {-0.25});                                               // 4 one haplotype: gap +inf
    b.add(3, 0, {}, {-4, -2.5, -9, 0, -3, -2.75, 0, 0, -8});                      // 5 no reads: V is the prior
    b.add(2, 2, {-3, nan, -3, -4}, {-2, -2, 0, -2});                              // 6 NaN
    b.add(2, 2, {-3, -4, -inf, -4}, {-2, -2, 0, -2});                             // 7 -inf
    b.add(2, 2, {-3, -4, -3, inf}, {-2, -2, 0, -2});                              // 8 +inf
    b.add(2, 2, {-3, -4, -3, -4.5}, {-2, -2, 0, -2}, {0, 0, 3, 0});               // 9 a pair that was not computed
    b.add(2, 1, {-3, -4}, {nan, -2, 0, -2});                                      // 10 NaN prior
    std::vector<double> many(size_t(DD_DIPPAIR_MAX_HAPS + 1), -1.0), manyp(size_t(DD_DIPPAIR_MAX_HAPS + 1) * (DD_DIPPAIR_MAX_HAPS + 1), -1.0);
    b.add(DD_DIPPAIR_MAX_HAPS + 1, 1, many, manyp);                               // 11 over the cap
    b.add(0, 0, {}, {});                                                          // 12 empty
    const size_t W = b.ho.size() - 1;
    Out o(W);
    CHECK(run(b, o, 1) == DD_SUCCESS);
    const int want[] = {DD_DIPPAIR_NO_HAPS, DD_DIPPAIR_CERTIFIED, DD_DIPPAIR_NO_HAPS, DD_DIPPAIR_TIE, DD_DIPPAIR_CERTIFIED, DD_DIPPAIR_CERTIFIED,
                        DD_DIPPAIR_NONFINITE, DD_DIPPAIR_NONFINITE, DD_DIPPAIR_NONFINITE, DD_DIPPAIR_NOT_COMPUTED, DD_DIPPAIR_NONFINITE,
                        DD_DIPPAIR_TOO_MANY_HAPS, DD_DIPPAIR_NO_HAPS};
    for (size_t w = 0; w < W; w++) {
        CHECK(o.state[w] == want[w]);
        if (want[w] != DD_DIPPAIR_CERTIFIED) CHECK(o.pair[2 * w] == -1 && o.pair[2 * w + 1] == -1);
        if (want[w] != DD_DIPPAIR_CERTIFIED && want[w] != DD_DIPPAIR_TIE) CHECK(o.best[w] == 0.0 && o.gap[w] == 0.0 && o.margin[w] == 0.0);
    }
    CHECK(o.pair[2] == 0 && o.pair[3] == 0 && near(o.best[1], -7.0) && near(o.gap[1], 0.5) && o.margin[1] > 0.0 && o.margin[1] < 1e-12);
    CHECK(o.gap[3] == 0.0 && o.margin[3] > 0.0 && near(o.best[3], -9.0));
    CHECK(o.pair[8] == 0 && o.pair[9] == 0 && std::isinf(o.gap[4]) && near(o.best[4], -11.25));
    CHECK(o.pair[10] == 0 && o.pair[11] == 1 && o.best[5] == -2.5 && o.gap[5] == 0.25);
    // threads change nothing; without status the uncomputed pair counts
    for (int t : {2, 5, 64}) {
        Out p(W);
        CHECK(run(b, p, t) == DD_SUCCESS);
        CHECK(p.pair == o.pair && p.state == o.state && p.best == o.best && p.gap == o.gap && p.margin == o.margin);
    }
    Out q(W);
    CHECK(run(b, q, 3, false) == DD_SUCCESS && q.state[9] == DD_DIPPAIR_CERTIFIED && q.pair[18] == 0 && q.pair[19] == 0);
    // a larger window at the cap, sums of 70 reads: the pair with the one better prior
    const int H = DD_DIPPAIR_MAX_HAPS, R = 70;
    Batch big;
    std::vector<double> l(size_t(H) * R), p(size_t(H) * H, -3.0);
    for (size_t i = 0; i < l.size(); i++) l[i] = -1.0 - double((i * 2654435761u) % 1000) / 37.0;
    for (int r = 0; r < R; r++) l[size_t(5) * R + r] = l[size_t(9) * R + r] = -0.5;
    p[size_t(5) * H + 9] = -2.0;
    big.add(H, R, l, p);
    Out ob(1);
    CHECK(run(big, ob, 1) == DD_SUCCESS && ob.state[0] == DD_DIPPAIR_CERTIFIED && ob.pair[0] == 5 && ob.pair[1] == 9 && near(ob.gap[0], 1.0));
    // validation
    dd_batch db = dd_batch();
    db.n_windows = 1;
    CHECK(dd_diploid_pairs_host(&db, NULL, NULL, NULL, &o.r, 1) == DD_ERR_INVALID);
    CHECK(dd_diploid_pairs_host(NULL, NULL, NULL, NULL, &o.r, 1) == DD_ERR_INVALID);
    if (adapter_checks()) { printf("diploid_pair_check: %d adapter checks failed\n", g_stub_failed); return 1; }
    printf("diploid_pair_check: ok\n");
    return 0;
}
