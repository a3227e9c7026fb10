// pooled_em_check — dd_pooled_em_host (csrc/pooled_em_host.cpp) and the host code around the loop (host/pooled_em.cpp) on their own: no
// GPU, no HIP header, standard library only.  tests/test_pooled_em_cpu.py builds it with g++ -fsanitize=address,undefined together with
// pooled_em_host.cpp, host/pooled_em.cpp and host/genotype.cpp (addLogs) and runs it directly.
// It runs the shapes of the GPU test (reads 0 ... 1000, haplotypes 1 ... 200, three masks, the four kinds of ll), on one thread and on
// several, and checks what must hold whatever the numbers: iteration counts in 2 ... 27, frequencies that sum to 1, finite outputs,
// the same bits from every thread count, untouched guard words around the outputs, and the rejection of malformed tables.  Then
// handmade windows (haplotypes with indels, SNPs and ignored "=>D" SNPs, candidates with and without a frequency, three pools, one of
// them empty, filtered haplotypes) go through plan, EM and lines for the three bayesTypes: one line per (candidate variant, pool).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../include/dindel_hmm.h"
#include "../dindel_tgi_amd/host/pooled_em_text.hpp"

namespace {
int failures = 0;
void expect(bool ok, const char *what, long a = 0, long b = 0)
{
    if (!ok) { printf("FAILED: %s (%ld, %ld)\n", what, a, b); failures++; }
}
uint64_t state = 0x9E3779B97F4A7C15ull;
double uniform(double lo, double hi)
{
    state ^= state << 13; state ^= state >> 7; state ^= state << 17;
    return lo + (hi - lo) * (double)(state >> 11) * (1.0 / 9007199254740992.0);
}
const double kGuard = -12345.678;
} // namespace

int main()
{
    const int reads[] = {0, 1, 2, 63, 64, 65, 128, 130, 1000}, haps[] = {1, 2, 8, 9, 33, 200};
    for (int content = 0; content < 4; content++) {
        std::vector<int32_t> who(1, 0), wro(1, 0), sw;
        std::vector<int64_t> so(1, 0);
        std::vector<double> ll;
        std::vector<uint8_t> compat;
        int w = 0;
        for (int nh : haps)
            for (int nr : reads) {
                if (content && nr == 1000 && nh > 9) continue;          // the sanitizers' slowdown: the largest windows once
                const size_t base = ll.size();
                for (int h = 0; h < nh; h++)
                    for (int r = 0; r < nr; r++) ll.push_back(content == 2 ? -20.0 : uniform(-150.0, -5.0));
                if (content == 1 && nr) for (int h = 0; h < nh; h++) ll[base + (size_t)h * nr + nr / 2] = -1e4;
                if (content == 3) for (int r = 0; r < nr; r++) ll[base + (size_t)(nh - 1) * nr + r] = -1e300;
                who.push_back(who.back() + nh); wro.push_back(wro.back() + nr);
                for (int m = 0; m < 3; m++) {
                    sw.push_back(w);
                    for (int h = 0; h < nh; h++) compat.push_back(m == 0 ? 1 : m == 1 ? h == (w + m) % nh : h % 2 == 0);
                    so.push_back(so.back() + nh);
                }
                w++;
            }
        dd_batch b;
        memset(&b, 0, sizeof(b));
        b.n_windows = w; b.win_hap_off = who.data(); b.win_read_off = wro.data();
        dd_pooled_slots s = {(int64_t)sw.size(), sw.data(), so.data(), compat.data()};
        const size_t N = sw.size(), F = (size_t)so.back();
        std::vector<double> lk[2], fr[2], ed[2];
        std::vector<int32_t> it[2];
        for (int pass = 0; pass < 2; pass++) {
            lk[pass].assign(N + 2, kGuard); fr[pass].assign(F + 2, kGuard); ed[pass].assign(N + 2, kGuard); it[pass].assign(N + 2, -77);
            dd_pooled_result out = {lk[pass].data() + 1, fr[pass].data() + 1, it[pass].data() + 1, ed[pass].data() + 1};
            const int rc = dd_pooled_em_host(&b, ll.data(), &s, content % 2 ? 1.0 : 0.001, 1e-4, &out, pass ? 5 : 1);
            expect(rc == DD_SUCCESS, "dd_pooled_em_host succeeds", rc, content);
            expect(lk[pass][0] == kGuard && lk[pass][N + 1] == kGuard && fr[pass][0] == kGuard && fr[pass][F + 1] == kGuard &&
                   ed[pass][0] == kGuard && ed[pass][N + 1] == kGuard && it[pass][0] == -77 && it[pass][N + 1] == -77, "guard words", content, pass);
        }
        expect(!memcmp(lk[0].data(), lk[1].data(), (N + 2) * 8) && !memcmp(fr[0].data(), fr[1].data(), (F + 2) * 8) &&
               !memcmp(ed[0].data(), ed[1].data(), (N + 2) * 8) && !memcmp(it[0].data(), it[1].data(), (N + 2) * 4), "one thread and five agree", content);
        for (size_t i = 0; i < N; i++) {
            expect(it[0][i + 1] >= 2 && it[0][i + 1] <= 27, "iterations in 2 ... 27", (long)i, it[0][i + 1]);
            expect(std::isfinite(lk[0][i + 1]) && lk[0][i + 1] <= 0.0 && std::isfinite(ed[0][i + 1]), "finite loglik and ediff", (long)i, content);
            double sum = 0.0;
            for (int64_t k = so[i]; k < so[i + 1]; k++) { sum += fr[0][k + 1]; expect(fr[0][k + 1] >= 0.0 && fr[0][k + 1] <= 1.0, "frequency in [0, 1]", (long)i); }
            expect(std::fabs(sum - 1.0) < 1e-12, "frequencies sum to 1", (long)i, content);
        }
        if (content == 0) {             // malformed tables are refused before anything is read
            dd_pooled_result out = {lk[0].data(), fr[0].data(), it[0].data(), ed[0].data()};
            std::vector<int32_t> bad_sw(sw); bad_sw[3] = w;
            dd_pooled_slots s2 = {(int64_t)N, bad_sw.data(), so.data(), compat.data()};
            expect(dd_pooled_em_host(&b, ll.data(), &s2, 0.001, 1e-4, &out, 1) == DD_ERR_INVALID, "a slot outside the batch is refused");
            std::vector<int64_t> bad_so(so); bad_so[5] += 1;
            dd_pooled_slots s3 = {(int64_t)N, sw.data(), bad_so.data(), compat.data()};
            expect(dd_pooled_em_host(&b, ll.data(), &s3, 0.001, 1e-4, &out, 1) == DD_ERR_INVALID, "slot_off that does not fit is refused");
            expect(dd_pooled_em_host(&b, ll.data(), &s, 0.0, 1e-4, &out, 1) == DD_ERR_INVALID, "a0 = 0 is refused");
            expect(dd_pooled_em_host(&b, nullptr, &s, 0.001, 1e-4, &out, 1) == DD_ERR_INVALID, "null ll is refused");
        }
    }
    // host/pooled_em.cpp on handmade windows
    for (int variant = 0; variant < 4; variant++) {
        std::ostringstream w;
        const int nr = variant == 3 ? 0 : 37 + variant, nh = 6;
        w << "W 3 20 5000 5120 5060 3\nC 5060 -AC -1\nC 5060 +GAT 0.02\nC 5040 A=>G 0.3\nC 5090 C=>D 0.5\n";
        const char *vars[6] = {"V 60 *REF\n", "V 60 -AC\n", "V 60 +GAT\nV 75 *REF\n", "V 40 A=>G\nV 60 -AC\n", "V 60 *REF\nV 90 C=>D\n", "V 60 *REF\nV 100 +T\n"};
        for (int h = 0; h < nh; h++) w << "H " << (variant == 1 && h == 2 ? 1 : variant == 2 && (h == 0 || h == 3) ? 1 : 0) << "\n" << vars[h];
        for (int r = 0; r < nr; r++) w << "R " << (r % 5 != 0) << " " << (r % 3 == 0) << " " << (r % 2 ? 0.9999 : 0.99) << " " << (r % 11 == 3) << "\n";
        for (int h = 0; h < nh; h++)
            for (int r = 0; r < nr; r++) {
                w << "L " << h << " " << r << " " << uniform(-60.0, -5.0) << " " << (r % 7 == 0) << "\n";
                if ((h + r) % 3) w << "K " << h << " " << r << " 60 0\nK " << h << " " << r << " 40 1\n";
            }
        w << "X 60 -AC 7 5\nX 40 A=>G 2 2\n";
        const char *programs[3] = {"all", "singlevariant", "priorpersite"};
        for (int p = 0; p < 3; p++) {
            std::string lines;
            try { lines = dindel::pooledLinesOfText(w.str(), programs[p], p == 1 ? 1.0 : 0.001, 1e-3, 1e-4); }
            catch (std::string &e) { printf("threw: %s\n", e.c_str()); expect(false, "pooledLinesOfText throws", variant, p); }
            long n = 0;
            for (size_t i = 0; i < lines.size(); i++) n += lines[i] == '\n';
            expect(n == 9, "one line per (candidate variant, pool)", n, variant * 10 + p);
            expect(lines.find(" nan") == std::string::npos || nr == 0, "no nan cell", variant, p);
        }
    }
    bool refused = false;
    try { dindel::pooledLinesOfText("W 1 20 1 2 1 1\nV 3 -A\n", "all", 0.001, 1e-3, 1e-4); } catch (std::string &) { refused = true; }
    expect(refused, "a malformed window text is refused");
    // the functions at their edges
    const double x[] = {-1e308, -745.2, -708.4, -1e-320, 0.0, 1e-320, 709.9, 1e308};
    double y[8];
    expect(dd_pooled_math_eval(0, x, y, 8) == DD_SUCCESS && y[0] == 0.0 && y[2] == 0.0 && y[4] == 1.0 && std::isinf(y[7]), "exp at its edges");
    expect(dd_pooled_math_eval(1, x, y, 8) == DD_SUCCESS && std::isnan(y[0]) && std::isinf(y[4]) && std::fabs(y[5] + 737.0) < 1.0, "log at its edges");
    expect(dd_pooled_math_eval(2, x, y, 8) == DD_SUCCESS && std::isnan(y[4]) && y[5] < -1e300 && std::fabs(y[6] - std::log(709.9)) < 1e-3, "digamma at its edges");
    if (failures) { printf("pooled_em_check: %d failures\n", failures); return 1; }
    printf("pooled_em_check: ok\n");
    return 0;
}
