// audit_faster_check.cpp — the host arithmetic of an audit of the --faster model on its own, for a build under AddressSanitizer and UBSan
// (tests/test_audit_faster_cpu.py compiles it with csrc/faster_shadow_host.cpp, csrc/audit_host.cpp, csrc/batch_host.cpp and csrc/plan.cpp,
// host code only, and runs it as a program; no GPU, no HIP call).  Seeded random batches — windows without reads or haplotypes, long
// windows, reads of 1 ... 60 bp (some shorter than a k-mer), haplotypes shorter than maxLengthDel, non-ACGT bytes, haplotypes with and
// without variants and flanks — go through dd_audit_select_faster with every kind of n_want; the CPU shadow (dd_audit_shadow_faster_host)
// is written into buffers of exactly the sample's lengths (the sanitizer sees any element touched outside them) and compared by
// dd_audit_compare_host_faster with the shadow of the whole batch, clean and with planted differences, with record caps of 0, 1 and more.
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
    std::vector<uint32_t> win_hap_start, read_start;
    std::vector<uint8_t> qidx, mqidx;
    std::vector<double> quals, mapqs;
    std::string hap_seq, read_seq;
    dd_batch b;
};

void make_batch(std::mt19937_64 &rng, Batch &B, int W, bool with_vars)
{
    auto below = [&](int n) { return (int)(rng() % (uint64_t)n); };
    const char *alphabet = "ACGTACGTACGTACGTNnacR";
    B.win_hap_off.assign(1, 0); B.win_read_off.assign(1, 0); B.hap_seq_off.assign(1, 0); B.read_seq_off.assign(1, 0); B.hap_var_off.assign(1, 0);
    B.quals = {0.999, 0.99, 0.9, 0.5}; B.mapqs = {0.9999, 0.99999, 0.9, 0.5};
    for (int w = 0; w < W; w++) {
        const int kind = below(12);
        const int H = kind == 0 ? 0 : 1 + below(3), R = kind == 1 ? 0 : 1 + below(5);
        const int base = kind == 3 ? 2 + below(6) : 20 + below(120);              // kind 3: around maxLengthDel and the k-mer length
        std::string ref;
        for (int i = 0; i < base + 12; i++) ref.push_back(kind == 4 ? "AC"[i & 1] : alphabet[below(21)]);   // kind 4: a tandem repeat
        for (int h = 0; h < H; h++) {
            const int len = kind == 2 ? 767 + below(40) : base + below(12);        // kind 2: beyond dd_faster_kernel's limit
            for (int i = 0; i < len; i++) B.hap_seq.push_back(i < (int)ref.size() ? ref[(size_t)i] : "ACGT"[below(4)]);
            B.hap_seq_off.push_back((int32_t)B.hap_seq.size());
            const int nv = with_vars ? below(3) : 0;
            for (int v = 0; v < nv; v++) {
                const int s = below(len), e = s + below(4);
                B.hap_var.push_back(s); B.hap_var.push_back(e);
                B.flank.push_back(s - below(8)); B.flank.push_back(e + below(8)); B.flank.push_back(below(3));
            }
            B.hap_var_off.push_back((int32_t)(B.hap_var.size() / 2));
        }
        for (int r = 0; r < R; r++) {
            const int len = 1 + below(kind == 5 ? 6 : 60), at = below((int)ref.size());
            for (int i = 0; i < len; i++) {
                B.read_seq.push_back(below(20) ? ref[(size_t)(at + i) % ref.size()] : alphabet[below(21)]);
                B.qidx.push_back((uint8_t)below(4));
            }
            B.read_seq_off.push_back((int32_t)B.read_seq.size());
            B.mqidx.push_back((uint8_t)below(4));
            B.read_start.push_back(1000u + (uint32_t)at + (uint32_t)below(3) * 400u - 400u);   // left of, inside and right of the window
        }
        B.win_hap_off.push_back(B.win_hap_off.back() + H);
        B.win_read_off.push_back(B.win_read_off.back() + R);
        B.win_hap_start.push_back(1000u);
    }
    B.qidx.push_back(0); B.mqidx.push_back(0); B.read_start.push_back(0);          // (never empty: data() of an empty vector may be NULL)
    std::memset(&B.b, 0, sizeof(B.b));
    B.b.n_windows = W;
    B.b.win_hap_off = B.win_hap_off.data(); B.b.win_read_off = B.win_read_off.data(); B.b.win_hap_start = B.win_hap_start.data();
    B.b.hap_seq_off = B.hap_seq_off.data(); B.b.hap_seq = B.hap_seq.data();
    B.b.read_seq_off = B.read_seq_off.data(); B.b.read_seq = B.read_seq.data();
    B.b.read_qidx = B.qidx.data(); B.b.read_mqidx = B.mqidx.data(); B.b.read_start = B.read_start.data();
    B.b.n_qual = 4; B.b.qual_table = B.quals.data(); B.b.n_mapq = 4; B.b.mapq_table = B.mapqs.data();
    if (with_vars) {
        B.hap_var.push_back(0); B.flank.push_back(0);
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
        for (auto &v : d) v.assign((size_t)n_pairs, 7.0);
        for (auto &v : u8) v.assign((size_t)n_pairs, 7);
        for (auto &v : i16) v.assign((size_t)n_pairs, 7);
        for (auto &v : cov) v.assign((size_t)cov_len, 7);
        hpos.assign((size_t)hpos_len, 7);
        status.assign((size_t)n_pairs, 7);
        std::memset(&r, 0, sizeof(r));
        r.ll = d[0].data(); r.llOn = d[1].data(); r.llOff = d[2].data(); r.mLogBQ = d[3].data();
        r.offHap = u8[0].data(); r.offHapHMQ = u8[1].data();
        int16_t **f[] = {&r.numIndels, &r.numMismatch, &r.nBQT, &r.nmmBQT, &r.nMMLeft, &r.nMMRight, &r.firstBase, &r.lastBase};
        for (int i = 0; i < 8; i++) *f[i] = i16[i].data();
        r.hpos = hpos.data(); r.var_covered = cov[0].data(); r.var_fcov = cov[1].data(); r.status = status.data();
    }
};

dd_audit_view view_of(int W, std::vector<uint8_t> &cls, std::vector<int64_t> &po, std::vector<int64_t> &ho, std::vector<int64_t> &vo, const dd_audit_sizes &sz)
{
    dd_audit_view v;
    std::memset(&v, 0, sizeof(v));
    v.n_windows = W; v.n_qual = 4;
    v.audit_class = cls.data(); v.pair_off = po.data(); v.hpos_off = ho.data(); v.varcov_off = vo.data(); v.sizes = sz;
    return v;
}

void one_batch(uint64_t seed, bool with_vars)
{
    std::mt19937_64 rng(seed);
    Batch B;
    const int W = 1 + (int)(rng() % 24);
    make_batch(rng, B, W, with_vars);
    dd_params p;
    dd_params_cli_defaults(&p);
    p.maxLengthDel = (int32_t)(seed % 3 == 0 ? 3 : 5);
    std::vector<uint8_t> cls((size_t)W), audit((size_t)W), all((size_t)W);
    int32_t mx[4];
    CHECK(dd_screen_windows_ex(&p, &B.b, DD_OPT_LONG_WINDOWS_FASTER, cls.data(), mx) >= 0);
    std::vector<int64_t> po((size_t)W + 1), ho((size_t)W + 1), vo((size_t)W + 1), fpo((size_t)W + 1), fho((size_t)W + 1), fvo((size_t)W + 1);
    // the "primary": the shadow of every eligible window, which lies where dd_batch_offsets puts it when every window with pairs is chosen
    dd_audit_sizes fsz;
    const int E = dd_audit_select_faster(&p, &B.b, cls.data(), DD_OPT_LONG_WINDOWS_FASTER, 1, W, all.data(), fpo.data(), fho.data(), fvo.data(), &fsz);
    CHECK(E >= 0 && E <= W && fsz.n_windows == E);
    std::vector<int64_t> bpo((size_t)W + 1), bho((size_t)W + 1), bvo((size_t)W + 1);
    CHECK(dd_batch_offsets(&B.b, bpo.data(), bho.data(), bvo.data()) == DD_SUCCESS);
    bool every = true;
    for (int w = 0; w < W; w++) every = every && (all[(size_t)w] == DD_WIN_LONG || bpo[(size_t)w + 1] == bpo[(size_t)w]);
    CHECK(every);                                   // (no window of these batches is beyond the long limits)
    CHECK(bpo == fpo);
    Results P;
    P.size(bpo[(size_t)W], bho[(size_t)W], bvo[(size_t)W]);
    dd_audit_view fv = view_of(W, all, fpo, fho, fvo, fsz);
    // offsets of hpos / coverage in the full layout also count windows with haplotypes and reads only: equal when all such are chosen
    CHECK(fpo[(size_t)W] == bpo[(size_t)W] && fho[(size_t)W] == bho[(size_t)W] && fvo[(size_t)W] == bvo[(size_t)W]);
    CHECK(dd_audit_shadow_faster_host(&p, &B.b, &fv, &P.r) == DD_SUCCESS);

    const int wants[] = {0, 1, 3, W / 2, W, W + 5, -2};
    for (int want : wants)
        for (uint32_t options : {0u, (uint32_t)DD_OPT_LONG_WINDOWS_FASTER}) {
            dd_audit_sizes sz;
            const int El = dd_audit_select_faster(&p, &B.b, cls.data(), options, seed * 31 + (uint64_t)want, want, audit.data(), po.data(), ho.data(), vo.data(), &sz);
            CHECK(El >= 0 && El <= E);
            const int expect = want <= 0 ? 0 : want >= El ? El : want;
            CHECK(sz.n_windows == expect);
            int64_t np = 0, nh = 0, nc = 0;
            int n = 0;
            for (int w = 0; w < W; w++) {
                CHECK(po[(size_t)w] == np && ho[(size_t)w] == nh && vo[(size_t)w] == nc);
                if (audit[(size_t)w] != DD_WIN_LONG) continue;
                n++;
                CHECK((cls[(size_t)w] == DD_WIN_MAIN || (options && cls[(size_t)w] == DD_WIN_LONG)) && bpo[(size_t)w + 1] > bpo[(size_t)w]);
                np += bpo[(size_t)w + 1] - bpo[(size_t)w]; nh += bho[(size_t)w + 1] - bho[(size_t)w]; nc += bvo[(size_t)w + 1] - bvo[(size_t)w];
            }
            CHECK(n == expect && sz.n_pairs == np && sz.hpos_len == nh && sz.var_cov_len == nc);
            Results S;
            S.size(sz.n_pairs, sz.hpos_len, sz.var_cov_len);
            dd_audit_view v = view_of(W, audit, po, ho, vo, sz);
            CHECK(dd_audit_shadow_faster_host(&p, &B.b, &v, &S.r) == DD_SUCCESS);
            for (int cap : {0, 1, 8}) {
                std::vector<unsigned char> rep(DD_AUDIT_REPORT_BYTES(cap));
                CHECK(dd_audit_compare_host_faster(&B.b, &P.r, &v, &S.r, rep.data(), cap) == DD_SUCCESS);
                dd_audit_report h;
                std::memcpy(&h, rep.data(), sizeof(h));
                CHECK(h.n_pairs == sz.n_pairs && h.n_diff == 0 && h.compared[DD_AUDIT_FIELD_status] == sz.n_pairs);
                if (h.n_diff && cap >= 1) {
                    dd_audit_record r0;
                    std::memcpy(&r0, rep.data() + sizeof(h), sizeof(r0));
                    std::printf("  seed %llu want %d: %lld differences, the first: window %d field %d pair %lld index %lld %llx / %llx\n", (unsigned long long)seed, want,
                                (long long)h.n_diff, r0.window, r0.field, (long long)r0.pair, (long long)r0.index, (unsigned long long)r0.primary_bits,
                                (unsigned long long)r0.shadow_bits);
                }
                if (sz.n_pairs == 0) continue;
                // plant: ll of the shadow's first and last pair, and the last hpos entry of the last pair if it is compared
                const size_t last = (size_t)sz.n_pairs - 1;
                const double ll_first = S.d[0][0], ll_last = S.d[0][last];
                S.d[0][0] += 1.0;
                if (last) S.d[0][last] += 1.0;
                const bool hp = S.status[last] == DD_PAIR_OK && !S.hpos.empty();
                if (hp) S.hpos.back() ^= 1;
                CHECK(dd_audit_compare_host_faster(&B.b, &P.r, &v, &S.r, rep.data(), cap) == DD_SUCCESS);
                std::memcpy(&h, rep.data(), sizeof(h));
                const int64_t planted = 1 + (last ? 1 : 0) + (hp ? 1 : 0);
                CHECK(h.n_diff == planted && h.diff[DD_AUDIT_FIELD_ll] == 1 + (last ? 1 : 0) && h.diff[DD_AUDIT_FIELD_hpos] == (hp ? 1 : 0));
                if (cap >= 1) {
                    dd_audit_record r0;
                    std::memcpy(&r0, rep.data() + sizeof(h), sizeof(r0));
                    CHECK(r0.field == DD_AUDIT_FIELD_ll && audit[(size_t)r0.window] == DD_WIN_LONG && r0.pair == bpo[(size_t)r0.window] && r0.index == r0.pair);
                }
                S.d[0][0] = ll_first;                  // (put back, not subtracted: the sums are rounded)
                S.d[0][last] = ll_last;
                if (hp) S.hpos.back() ^= 1;
            }
        }
}
} // namespace

int main()
{
    for (uint64_t seed = 1; seed <= 40; seed++) one_batch(seed, seed % 3 != 0);
    if (g_failed) { std::printf("audit_faster_check: %d check(s) failed\n", g_failed); return 1; }
    std::printf("audit_faster_check: ok\n");
    return 0;
}
