// audit_check.cpp — the host arithmetic of an audit on its own, for a build under AddressSanitizer and UBSan (tests/test_audit_cpu.py
// compiles it with csrc/audit_host.cpp, csrc/batch_host.cpp and csrc/plan.cpp, host code only, and runs it as a program; no GPU, no HIP call).
// Seeded random batches — windows without reads or haplotypes, screened windows, haplotypes with and without variants — go through
// dd_audit_select with every kind of n_want; the offsets and sizes are recomputed here; a shadow compacted from random "results" goes through
// dd_audit_compare_host in buffers of exactly the sample's lengths (the sanitizer sees any element read outside them), clean and with
// planted differences, with record caps of 0, 1 and more than the differences.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../include/dindel_hmm.h"

namespace {
int g_failed = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); g_failed++; } } while (0)

struct Batch {
    std::vector<int32_t> win_hap_off, win_read_off, hap_seq_off, read_seq_off, hap_var_off, hap_var, flank;
    std::vector<uint32_t> win_hap_start;
    std::string hap_seq, read_seq;
    dd_batch b;
};

void make_batch(std::mt19937_64 &rng, Batch &B, int W, bool with_vars)
{
    auto below = [&](int n) { return (int)(rng() % (uint64_t)n); };
    B.win_hap_off.assign(1, 0); B.win_read_off.assign(1, 0); B.hap_seq_off.assign(1, 0); B.read_seq_off.assign(1, 0); B.hap_var_off.assign(1, 0);
    B.hap_var.clear(); B.flank.clear(); B.hap_seq.clear(); B.read_seq.clear(); B.win_hap_start.clear();
    for (int w = 0; w < W; w++) {
        const int kind = below(10);
        const int H = kind == 0 ? 0 : 1 + below(4), R = kind == 1 ? 0 : 1 + below(6);
        const int base = 20 + below(300);
        for (int h = 0; h < H; h++) {
            const int len = kind == 2 ? 800 + below(100) : base + below(12);     // kind 2: beyond the main kernels' limit
            B.hap_seq.append((size_t)len, "ACGT"[below(4)]);
            B.hap_seq_off.push_back((int32_t)B.hap_seq.size());
            const int nv = with_vars ? below(3) : 0;
            for (int v = 0; v < nv; v++) {
                B.hap_var.push_back(below(len)); B.hap_var.push_back(below(len));
                B.flank.push_back(0); B.flank.push_back(len - 1); B.flank.push_back(1 + below(2));
            }
            B.hap_var_off.push_back((int32_t)(B.hap_var.size() / 2));
        }
        for (int r = 0; r < R; r++) {
            B.read_seq.append((size_t)(1 + below(60)), 'A');
            B.read_seq_off.push_back((int32_t)B.read_seq.size());
        }
        B.win_hap_off.push_back(B.win_hap_off.back() + H);
        B.win_read_off.push_back(B.win_read_off.back() + R);
        B.win_hap_start.push_back(1000u);
    }
    std::memset(&B.b, 0, sizeof(B.b));
    B.b.n_windows = W;
    B.b.win_hap_off = B.win_hap_off.data(); B.b.win_read_off = B.win_read_off.data(); B.b.win_hap_start = B.win_hap_start.data();
    B.b.hap_seq_off = B.hap_seq_off.data(); B.b.hap_seq = B.hap_seq.data();
    B.b.read_seq_off = B.read_seq_off.data(); B.b.read_seq = B.read_seq.data();
    if (with_vars) {
        B.hap_var.push_back(0); B.flank.push_back(0);                      // (never empty: data() of an empty vector may be NULL)
        B.b.hap_var_off = B.hap_var_off.data(); B.b.hap_var = B.hap_var.data(); B.b.hap_var_flank = B.flank.data();
    }
}

// exact-size buffers: one allocation per array, so that the sanitizer catches an index one past the end
struct Results {
    std::vector<double> d[4];
    std::vector<uint8_t> u8[2], cov[2];
    std::vector<int16_t> i16[8], hpos;
    std::vector<int32_t> status;
    dd_result r;
    void size(int64_t n_pairs, int64_t hpos_len, int64_t cov_len)
    {
        for (auto &v : d) v.assign((size_t)n_pairs, 0.0);
        for (auto &v : u8) v.assign((size_t)n_pairs, 0);
        for (auto &v : i16) v.assign((size_t)n_pairs, 0);
        for (auto &v : cov) v.assign((size_t)cov_len, 0);
        hpos.assign((size_t)hpos_len, 0);
        status.assign((size_t)n_pairs, 0);
        std::memset(&r, 0, sizeof(r));
        r.ll = d[0].data(); r.llOn = d[1].data(); r.llOff = d[2].data(); r.mLogBQ = d[3].data();
        r.offHap = u8[0].data(); r.offHapHMQ = u8[1].data();
        int16_t **f[] = {&r.numIndels, &r.numMismatch, &r.nBQT, &r.nmmBQT, &r.nMMLeft, &r.nMMRight, &r.firstBase, &r.lastBase};
        for (int i = 0; i < 8; i++) *f[i] = i16[i].data();
        r.hpos = hpos.data(); r.var_covered = cov[0].data(); r.var_fcov = cov[1].data(); r.status = status.data();
    }
};

// memcpy that takes an empty (possibly NULL) range
void copy(void *dst, const void *src, size_t n) { if (n) std::memcpy(dst, src, n); }

void one_batch(uint64_t seed, bool with_vars)
{
    std::mt19937_64 rng(seed);
    Batch B;
    const int W = 1 + (int)(rng() % 40);
    make_batch(rng, B, W, with_vars);
    dd_params p;
    dd_params_cli_defaults(&p);
    std::vector<uint8_t> cls((size_t)W), audit((size_t)W);
    int32_t mx[2];
    CHECK(dd_screen_windows(&B.b, cls.data(), mx) >= 0);
    std::vector<int64_t> po((size_t)W + 1), ho((size_t)W + 1), vo((size_t)W + 1), fpo((size_t)W + 1), fho((size_t)W + 1), fvo((size_t)W + 1);
    CHECK(dd_batch_offsets(&B.b, fpo.data(), fho.data(), fvo.data()) == DD_SUCCESS);
    Results P;
    P.size(fpo[(size_t)W], fho[(size_t)W], fvo[(size_t)W]);
    for (size_t i = 0; i < P.status.size(); i++) {
        const int k = (int)(rng() % 8);
        P.status[i] = k == 0 ? DD_PAIR_HAPSIZE : k == 1 ? DD_PAIR_NAN : DD_PAIR_OK;
        P.d[0][i] = -(double)(rng() % 1000);
        P.i16[7][i] = (int16_t)(rng() % 100);
    }
    for (auto &v : P.hpos) v = (int16_t)(rng() % 300);
    for (auto &v : P.cov[0]) v = (uint8_t)(rng() % 2);

    const int wants[] = {0, 1, 3, W / 2, W, W + 5, -2};
    for (int want : wants) {
        dd_audit_sizes sz;
        const int E = dd_audit_select(&p, &B.b, cls.data(), seed * 31 + (uint64_t)want, want, audit.data(), po.data(), ho.data(), vo.data(), &sz);
        CHECK(E >= 0 && E <= W);
        const int expect = want <= 0 ? 0 : want >= E ? E : want;
        CHECK(sz.n_windows == expect);
        int64_t np = 0, nh = 0, nc = 0;
        int n = 0;
        for (int w = 0; w < W; w++) {
            CHECK(po[(size_t)w] == np && ho[(size_t)w] == nh && vo[(size_t)w] == nc);
            CHECK(audit[(size_t)w] == DD_WIN_LONG || audit[(size_t)w] == DD_WIN_UNSUPPORTED);
            if (audit[(size_t)w] != DD_WIN_LONG) continue;
            n++;
            CHECK(cls[(size_t)w] == 0 && fpo[(size_t)w + 1] > fpo[(size_t)w]);
            np += fpo[(size_t)w + 1] - fpo[(size_t)w]; nh += fho[(size_t)w + 1] - fho[(size_t)w]; nc += fvo[(size_t)w + 1] - fvo[(size_t)w];
        }
        CHECK(n == expect && po[(size_t)W] == np && sz.n_pairs == np && sz.hpos_len == nh && sz.var_cov_len == nc);

        // the shadow: the chosen windows' pieces of the primary, in buffers of exactly the sample's lengths
        Results S;
        S.size(sz.n_pairs, sz.hpos_len, sz.var_cov_len);
        for (int w = 0; w < W; w++) {
            if (audit[(size_t)w] != DD_WIN_LONG) continue;
            const size_t a = (size_t)fpo[(size_t)w], c = (size_t)(fpo[(size_t)w + 1] - fpo[(size_t)w]), at = (size_t)po[(size_t)w];
            for (int k = 0; k < 4; k++) copy(S.d[k].data() + at, P.d[k].data() + a, c * 8);
            for (int k = 0; k < 2; k++) copy(S.u8[k].data() + at, P.u8[k].data() + a, c);
            for (int k = 0; k < 8; k++) copy(S.i16[k].data() + at, P.i16[k].data() + a, c * 2);
            copy(S.status.data() + at, P.status.data() + a, c * 4);
            copy(S.hpos.data() + ho[(size_t)w], P.hpos.data() + fho[(size_t)w], (size_t)(fho[(size_t)w + 1] - fho[(size_t)w]) * 2);
            for (int k = 0; k < 2; k++)
                copy(S.cov[k].data() + vo[(size_t)w], P.cov[k].data() + fvo[(size_t)w], (size_t)(fvo[(size_t)w + 1] - fvo[(size_t)w]));
        }
        dd_audit_view v;
        std::memset(&v, 0, sizeof(v));
        v.n_windows = W; v.n_qual = 1;
        v.audit_class = audit.data(); v.pair_off = po.data(); v.hpos_off = ho.data(); v.varcov_off = vo.data(); v.sizes = sz;
        for (int cap : {0, 1, 8}) {
            std::vector<unsigned char> rep(DD_AUDIT_REPORT_BYTES(cap));
            CHECK(dd_audit_compare_host(&B.b, &P.r, &v, &S.r, rep.data(), cap) == DD_SUCCESS);
            dd_audit_report h;
            std::memcpy(&h, rep.data(), sizeof(h));
            CHECK(h.n_pairs == sz.n_pairs && h.n_diff == 0 && h.compared[DD_AUDIT_FIELD_status] == sz.n_pairs);
            if (sz.n_pairs == 0) continue;
            // plant: ll of the shadow's first and last pair, and the last hpos entry of the last pair if it is compared
            const size_t last = (size_t)sz.n_pairs - 1;
            S.d[0][0] += 1.0;
            if (last) S.d[0][last] += 1.0;
            const bool hp = S.status[last] != DD_PAIR_HAPSIZE && !S.hpos.empty();
            if (hp) S.hpos.back() ^= 1;
            CHECK(dd_audit_compare_host(&B.b, &P.r, &v, &S.r, rep.data(), cap) == DD_SUCCESS);
            std::memcpy(&h, rep.data(), sizeof(h));
            const int64_t planted = 1 + (last ? 1 : 0) + (hp ? 1 : 0);
            CHECK(h.n_diff == planted && h.diff[DD_AUDIT_FIELD_ll] == 1 + (last ? 1 : 0) && h.diff[DD_AUDIT_FIELD_hpos] == (hp ? 1 : 0));
            if (cap >= 1) {
                dd_audit_record r0;
                std::memcpy(&r0, rep.data() + sizeof(h), sizeof(r0));
                CHECK(r0.field == DD_AUDIT_FIELD_ll && audit[(size_t)r0.window] == DD_WIN_LONG && r0.pair == fpo[(size_t)r0.window] && r0.index == r0.pair);
            }
            S.d[0][0] -= 1.0;
            if (last) S.d[0][last] -= 1.0;
            if (hp) S.hpos.back() ^= 1;
        }
    }
}
} // namespace

int main()
{
    for (uint64_t seed = 1; seed <= 60; seed++) one_batch(seed, seed % 3 != 0);
    if (g_failed) { std::printf("audit_check: %d check(s) failed\n", g_failed); return 1; }
    std::printf("audit_check: ok\n");
    return 0;
}
