// batch_host.cpp — the batch bookkeeping of the C ABI: sizes, window screens, offsets, host tables, launch classes of a ragged batch,
// the partition for several devices.  O(bases) host work: nothing here calls the HIP runtime.
#include <cmath>
#include "capi_internal.h"

namespace ddh {
thread_local std::string g_err;

// ReadIndelErrorModel::getViterbiHPError — reference ReadIndelErrorModel.hpp:36-50
static double hp_error(int hpLen)
{
    static const double base[10] = {2.9e-5, 2.9e-5, 2.9e-5, 2.9e-5, 4.3e-5, 1.1e-4, 2.4e-4, 5.7e-4, 1.0e-3, 1.4e-3};
    int len = hpLen < 1 ? 1 : hpLen;
    double pbe = (len <= 10) ? base[len - 1] : base[9] + 4.3e-4 * double(len - 10);
    pbe *= double(hpLen);
    if (pbe > 0.99) pbe = 0.99;
    return pbe;
}

// the four offset arrays every walk over the windows needs
static int check_offset_arrays(const dd_batch *b)
{
    if (b->n_windows < 0 || !b->win_hap_off || !b->win_read_off || !b->hap_seq_off || !b->read_seq_off)
        return fail(DD_ERR_INVALID, "null offset array");
    return DD_SUCCESS;
}
// byte -> symbol id (dd_build_symbol_lut's rule).  Returns how many distinct haplotype bytes were left without an id (the 27th and later
// non-ACGTN values in byte order; they map to 31 like a byte no haplotype holds), or a DD_ERR_* code.
int assign_symbols(const dd_batch *b, uint8_t *out)
{
    if (!b || !out || !b->hap_seq_off || !b->win_hap_off) return fail(DD_ERR_INVALID, "null argument");
    for (int i = 0; i < 256; i++) out[i] = 31;                    // read-only symbol: equal to no haplotype symbol
    out[(unsigned char)'A'] = 0; out[(unsigned char)'C'] = 1; out[(unsigned char)'G'] = 2; out[(unsigned char)'T'] = 3;
    out[(unsigned char)'N'] = 4;
    bool seen[256] = {false};
    const int64_t n_haps = b->n_windows > 0 ? b->win_hap_off[b->n_windows] : 0;
    const int64_t nb = n_haps > 0 ? b->hap_seq_off[n_haps] : 0;
    if (nb > 0 && !b->hap_seq) return fail(DD_ERR_INVALID, "null input array");
    for (int64_t i = 0; i < nb; i++) seen[(unsigned char)b->hap_seq[i]] = true;
    int next = 5, left = 0;
    for (int c = 0; c < 256; c++) {
        if (!seen[c] || c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N') continue;
        if (next > 30) { left++; continue; }
        out[c] = (uint8_t)next++;
    }
    return left;
}

// what the screens need to know of one window
struct WinScan { int max_hap = 0, max_read = 0; bool empty_seq = false /* a length < 1 */, pairs = false /* it has haplotypes and reads */; };
static WinScan scan_window(const dd_batch *b, int w)
{
    WinScan s;
    for (int h = b->win_hap_off[w]; h < b->win_hap_off[w + 1]; h++) {
        const int len = b->hap_seq_off[h + 1] - b->hap_seq_off[h];
        if (len < 1) s.empty_seq = true;
        if (len > s.max_hap) s.max_hap = len;
    }
    for (int q = b->win_read_off[w]; q < b->win_read_off[w + 1]; q++) {
        const int len = b->read_seq_off[q + 1] - b->read_seq_off[q];
        if (len < 1) s.empty_seq = true;
        if (len > s.max_read) s.max_read = len;
    }
    s.pairs = b->win_hap_off[w + 1] > b->win_hap_off[w] && b->win_read_off[w + 1] > b->win_read_off[w];
    return s;
}

// The screen proper: win_class[w] = DD_WIN_MAIN for a window within main_hap / main_read, DD_WIN_LONG for one beyond them but within
// long_hap / long_read, else (or with an empty sequence, or — with_symbols — a haplotype byte that sym_lut left without an id)
// DD_WIN_UNSUPPORTED.  max_len_out[4] (may be NULL): longest haplotype / read among the main windows with pairs, then among the long ones.
// Returns the number of unsupported windows.
static int class_windows(const dd_batch *b, uint8_t *win_class, int32_t max_len_out[4], const uint8_t *sym_lut, bool with_symbols,
                         int main_hap, int main_read, int long_hap, int long_read)
{
    int n_bad = 0;
    int32_t m[4] = {0, 0, 0, 0};
    for (int w = 0; w < b->n_windows; w++) {
        const WinScan s = scan_window(b, w);
        bool bad = s.empty_seq || s.max_hap > long_hap || s.max_read > long_read;
        if (with_symbols && !bad) {
            const int64_t from = b->hap_seq_off[b->win_hap_off[w]], to = b->hap_seq_off[b->win_hap_off[w + 1]];
            for (int64_t i = from; i < to && !bad; i++)
                if (sym_lut[(unsigned char)b->hap_seq[i]] == 31) bad = true;   // a haplotype byte is never 31 unless it was left without an id
        }
        if (bad) { win_class[w] = DD_WIN_UNSUPPORTED; n_bad++; continue; }
        const bool is_long = s.max_hap > main_hap || s.max_read > main_read;
        win_class[w] = is_long ? DD_WIN_LONG : DD_WIN_MAIN;
        if (s.pairs) {
            int32_t *mm = m + (is_long ? 2 : 0);
            mm[0] = std::max(mm[0], s.max_hap); mm[1] = std::max(mm[1], s.max_read);
        }
    }
    if (max_len_out) memcpy(max_len_out, m, sizeof(m));
    return n_bad;
}

// sym_lut (may be NULL: lengths only) is assign_symbols' table; with_symbols: windows whose haplotypes hold a byte
// that got no id are skipped too (main model only: the --faster kernel compares the bytes themselves).
int screen_windows(const dd_batch *b, uint8_t *win_skip, int32_t max_len_out[2], const uint8_t *sym_lut, bool with_symbols)
{
    static_assert(DD_WIN_MAIN == 0 && DD_WIN_UNSUPPORTED == 1, "win_skip is the class without the long path");
    int32_t m[4];
    const int n = class_windows(b, win_skip, m, sym_lut, with_symbols, DD_MAX_HAP_LEN, DD_MAX_READ_LEN, DD_MAX_HAP_LEN, DD_MAX_READ_LEN);
    if (max_len_out) { max_len_out[0] = m[0]; max_len_out[1] = m[1]; }
    return n;
}

// Classes of the long-window option (dd_screen_windows_ex): 0 main kernels, 1 unsupported, 2 long path.  Without the option exactly
// screen_windows.  With it a window the main kernels cannot take — a haplotype > DD_MAX_HAP_LEN, a read > DD_MAX_READ_LEN, or on the D = 32
// build (maxLengthDel >= 12) a haplotype > 574 bp, which make_plan cannot place — goes to the long path when it is within the long limits.
int screen_windows_ex(const dd_params *p, const dd_batch *b, uint32_t options, uint8_t *win_class, int32_t max_len_out[4],
                      const uint8_t *sym_lut, bool with_symbols)
{
    if (options & DD_OPT_LONG_WINDOWS_FASTER)
        // classes for the --faster model: lengths only (it compares haplotype bytes, and maxLengthDel is only a size check there)
        return class_windows(b, win_class, max_len_out, sym_lut, false, DD_MAX_HAP_LEN, DD_MAX_READ_LEN, DD_LONG_MAX_HAP_LEN, DD_LONG_MAX_READ_LEN);
    if (!(options & DD_OPT_LONG_WINDOWS))
        return class_windows(b, win_class, max_len_out, sym_lut, with_symbols, DD_MAX_HAP_LEN, DD_MAX_READ_LEN, DD_MAX_HAP_LEN, DD_MAX_READ_LEN);
    if (wide_on(p, options))
        // maxLengthDel > 31 (DD_OPT_WIDE_DELETIONS): no main kernel build, every window within the long limits goes to the long path
        return class_windows(b, win_class, max_len_out, sym_lut, with_symbols, -1, -1, DD_LONG_MAX_HAP_LEN, DD_LONG_MAX_READ_LEN);
    const int main_hap_cap = pick_Dt(p->maxLengthDel + 1) > 12 ? kHapClasses[12].bound : DD_MAX_HAP_LEN;   // D = 32 build: K <= 9 (574 bp)
    return class_windows(b, win_class, max_len_out, sym_lut, with_symbols, main_hap_cap, DD_MAX_READ_LEN, DD_LONG_MAX_HAP_LEN, DD_LONG_MAX_READ_LEN);
}

// ---- launch classes of a ragged batch ----
// A launch = (lane tiling of the haplotypes, read class).  Reads up to 160 bp and longer ones are separate launches, as in round 3; the
// reads up to 160 bp of a tiling are cut once more where its launch plan changes — BY WINDOW: windows whose longest read still lets the
// back-pointer tile sit in LDS at full occupancy (<= T, from make_plan: ~115 bp at K = 2) are one launch, the other windows (all their
// reads up to 160 bp, short ones included) another — so windows of short reads keep the faster LDS build when a batch also holds 150-bp
// windows (one "<= 160 bp" launch put the 100-bp reads on the scratch build, 18 % slower), and no window pays the haplotype set-up in both
// (cutting by READ made the trimmed-read windows straddle the cut: 3.70e11 against 3.98e11 cells/s without the cut on bench.py's ragged
// batch).  A haplotype is listed in a launch only if its window has reads for it.
int build_launch_classes(const dd_batch *b, const uint8_t *win_skip, const dd_params *p, int32_t *list, dd_length_classes *out)
{
    dd_sizes sz;
    int rc = dd_batch_sizes(b, &sz);
    if (rc) return rc;
    memset(out, 0, sizeof(*out));
    const int W = b->n_windows;
    // pass 0: the folded builds (end states inside the generic candidate code, K <= 2 on the D = 6 build: +4.5 %) need every haplotype of their
    // launch to leave the last position idle — 64 K >= Hs + 3, i.e. up to 61 / 125 bp of the 62 / 126 the tiling holds.  One 126-bp haplotype
    // among thousands of shorter ones switched the fold off for all of them (the ragged leg's K = 2 launches).  When the haplotypes of exactly
    // the tiling's full length are few, they run apart (promote[c]): launches of their own, same tiling, not folded; the others fold.
    const Switches sw = read_switches();
    bool promote[DD_N_HAP_CLASSES] = {false};
    if (p && check_params(p) == DD_SUCCESS && pick_Dt(p->maxLengthDel + 1) == 6 && !sw.no_fold && !sw.no_promote) {
        int64_t n_fold[DD_N_HAP_CLASSES] = {0}, n_edge[DD_N_HAP_CLASSES] = {0};
        for (int w = 0; w < W; w++) {
            if (win_skip && win_skip[w]) continue;
            for (int64_t h = b->win_hap_off[w]; h < b->win_hap_off[w + 1]; h++) {
                const int len = b->hap_seq_off[h + 1] - b->hap_seq_off[h];
                const int c = hap_class_of(len < 1 ? 1 : (len > DD_MAX_HAP_LEN ? DD_MAX_HAP_LEN : len));
                if (len == kHapClasses[c].bound) n_edge[c]++; else n_fold[c]++;
            }
        }
        int used = 0, moved = 0;
        for (int c = 0; c < DD_N_HAP_CLASSES; c++) used += (n_fold[c] + n_edge[c]) > 0 ? 1 : 0;
        for (int c = 0; c < DD_N_HAP_CLASSES; c++) {
            int G0 = 1, K0 = 1;
            if (!pick_tiling(sw, kHapClasses[c].bound, 6, G0, K0)) continue;
            if (G0 != 1 || K0 > 2 || n_edge[c] == 0 || n_fold[c] == 0) continue;   // only the tilings that have a folded build
            // the full-length haplotypes get launches of their own (same tiling, not folded: they cost what they cost before); worth it when the
            // launch they leave behind is the bigger part — a small launch fills the chip badly
            promote[c] = n_edge[c] * 4 < n_fold[c] && (used + moved + 1) * DD_N_READ_CLASSES <= DD_N_HAP_CLASSES * DD_N_READ_CLASSES;
            moved += promote[c] ? 1 : 0;
        }
    }
    // internal class ids: 0 .. N-1 the tilings, N + c the full-length haplotypes of tiling c when they run apart
    constexpr int NC = 2 * DD_N_HAP_CLASSES;
    auto cls = [&](int len) { const int c = hap_class_of(len); return (promote[c] && len == kHapClasses[c].bound) ? DD_N_HAP_CLASSES + c : c; };
    // pass 1: haplotype class maxima (the read thresholds depend on the class' longest haplotype)
    int hmax[NC] = {0};
    bool any_skipped = false;
    for (int w = 0; w < W; w++) {
        if (win_skip && win_skip[w]) { any_skipped = any_skipped || b->win_hap_off[w + 1] > b->win_hap_off[w]; continue; }
        for (int64_t h = b->win_hap_off[w]; h < b->win_hap_off[w + 1]; h++) {
            const int len = b->hap_seq_off[h + 1] - b->hap_seq_off[h];
            if (len > DD_MAX_HAP_LEN) return fail(DD_ERR_UNSUPPORTED, "haplotype longer than 766 in a window that is not flagged in win_skip");
            const int c = cls(len < 1 ? 1 : len);
            if (len > hmax[c]) hmax[c] = len;
        }
    }
    int bound[NC][DD_N_READ_CLASSES];                        // upper read length of each interval of each tiling
    const bool one_read_class = sw.one_read_class;           // A/B: haplotype classes only
    for (int c = 0; c < NC; c++) {
        int T = hmax[c] > 0 ? lds_read_threshold(sw, p, hmax[c], b->n_qual) : 0;
        if (sw.read_bound >= 0) T = sw.read_bound;            // A/B only
        if (T < 1 || T >= 160) T = 0;
        bound[c][0] = one_read_class ? DD_MAX_READ_LEN : (T ? T : 160);
        bound[c][1] = one_read_class ? DD_MAX_READ_LEN : 160;
        bound[c][2] = DD_MAX_READ_LEN;
    }
    auto read_class = [&](int c, int len) { return len <= bound[c][0] ? 0 : (len <= bound[c][1] ? 1 : 2); };
    // pass 2: per window, which (tiling, interval) launches its haplotypes take part in
    struct Acc { std::vector<int32_t> haps; int max_hap = 0, max_read = 0, max_reads = 0; int64_t sum_reads = 0, n_win = 0, sum_len = 0; };
    std::vector<Acc> acc((size_t)NC * DD_N_READ_CLASSES);
    std::vector<int32_t> skipped;                             // haplotypes of skipped windows: marked by the first launch
    for (int w = 0; w < W; w++) {
        const int64_t h0 = b->win_hap_off[w], h1 = b->win_hap_off[w + 1], q0 = b->win_read_off[w], q1 = b->win_read_off[w + 1];
        if (win_skip && win_skip[w]) { for (int64_t h = h0; h < h1; h++) skipped.push_back((int32_t)h); continue; }
        if (h1 <= h0 || q1 <= q0) continue;
        unsigned seen = 0;                                    // tilings of this window already handled
        for (int64_t h = h0; h < h1; h++) {
            const int hl = b->hap_seq_off[h + 1] - b->hap_seq_off[h];
            const int c = cls(hl < 1 ? 1 : hl);
            if (seen & (1u << c)) continue;
            seen |= 1u << c;
            int cnt[DD_N_READ_CLASSES] = {0}, mx[DD_N_READ_CLASSES] = {0};
            int64_t sl[DD_N_READ_CLASSES] = {0};
            int mx160 = 0;                                        // the window's longest read up to 160 bp decides between classes 0 and 1
            for (int64_t q = q0; q < q1; q++) {
                const int len = b->read_seq_off[q + 1] - b->read_seq_off[q];
                if (len >= 1 && len <= bound[c][1] && len > mx160) mx160 = len;
            }
            const int k160 = read_class(c, mx160 > 0 ? mx160 : 1);
            for (int64_t q = q0; q < q1; q++) {
                const int len = b->read_seq_off[q + 1] - b->read_seq_off[q];
                if (len < 1) continue;
                const int k = len <= bound[c][1] ? k160 : 2;
                cnt[k]++;
                sl[k] += len;
                if (len > mx[k]) mx[k] = len;
            }
            for (int k = 0; k < DD_N_READ_CLASSES; k++) {
                if (!cnt[k]) continue;
                Acc &a = acc[(size_t)c * DD_N_READ_CLASSES + k];
                for (int64_t g = h; g < h1; g++) {
                    const int gl = b->hap_seq_off[g + 1] - b->hap_seq_off[g];
                    if (cls(gl < 1 ? 1 : gl) != c) continue;
                    a.haps.push_back((int32_t)g);
                    if (gl > a.max_hap) a.max_hap = gl;
                }
                if (mx[k] > a.max_read) a.max_read = mx[k];
                if (cnt[k] > a.max_reads) a.max_reads = cnt[k];
                a.sum_reads += cnt[k];
                a.sum_len += sl[k];
                a.n_win++;
            }
        }
    }
    int32_t off = 0;
    auto emit = [&](int c, int k, Acc &a, const std::vector<int32_t> *extra) {
        dd_launch_class &L = out->launch[out->n_launches++];
        L.list_off = off;
        if (extra && !extra->empty()) {                        // merge (both ascending) so that the list stays sorted
            std::vector<int32_t> m(a.haps.size() + extra->size());
            std::merge(a.haps.begin(), a.haps.end(), extra->begin(), extra->end(), m.begin());
            a.haps.swap(m);
        }
        L.list_len = (int32_t)a.haps.size();
        if (list) memcpy(list + off, a.haps.data(), a.haps.size() * sizeof(int32_t));
        off += L.list_len;
        L.hap_class = c % DD_N_HAP_CLASSES;
        L.max_hap_len = a.max_hap > 0 ? a.max_hap : 1;
        L.min_read_len = k == 2 ? bound[c][1] + 1 : 1;       // (class 1 = the windows with a read beyond T: all their reads up to 160 bp)
        L.max_read_len = a.max_read > 0 ? a.max_read : 1;
        L.max_window_reads = a.max_reads;
        L.avg_window_reads = a.n_win ? (int32_t)((a.sum_reads + a.n_win - 1) / a.n_win) : 0;
        L.avg_read_len = a.sum_reads ? (int32_t)(a.sum_len / a.sum_reads) : 0;
    };
    bool first = true;
    for (int c = 0; c < NC; c++)
        for (int k = 0; k < DD_N_READ_CLASSES; k++) {
            Acc &a = acc[(size_t)c * DD_N_READ_CLASSES + k];
            if (a.haps.empty()) continue;
            if (out->n_launches >= DD_N_HAP_CLASSES * DD_N_READ_CLASSES) return fail(DD_ERR_UNSUPPORTED, "more launch classes than dd_length_classes holds");
            emit(c, k, a, first ? &skipped : nullptr);
            first = false;
        }
    if (first && !skipped.empty()) {                           // nothing but skipped windows: one launch that only marks their pairs
        Acc a;
        emit(0, 0, a, &skipped);
    }
    out->list_len = off;
    return DD_SUCCESS;
}
} // namespace ddh
using namespace ddh;
extern "C" {
int dd_abi_version(void) { return DD_ABI_VERSION; }
const char *dd_last_error(void) { return g_err.c_str(); }

void dd_params_struct_defaults(dd_params *p)
{   // ObservationModelParameters::setDefaultValues — reference ObservationModel.hpp:39-64
    p->pError = 1e-4; p->pMut = 1e-4; p->pFirstgLO = 0.01; p->mapQualThreshold = 100.0;
    p->checkBaseQualThreshold = 0.95; p->maxLengthDel = 10; p->padCover = 5; p->bMid = -1;
    p->forceReadOnHaplotype = 0; p->mapUnmappedReads = 0; p->maxMismatch = 1; p->capMapQualFast = 40.0;
}
void dd_params_cli_defaults(dd_params *p)
{   // what main() installs — reference DInDel.cpp:3937-3949 with the option defaults at :4122-4157
    dd_params_struct_defaults(p);
    p->pError = 5e-4; p->pMut = 1e-5; p->maxLengthDel = 5; p->mapQualThreshold = 100.0; p->padCover = 2; p->maxMismatch = 2; p->capMapQualFast = 45.0;
}

int dd_batch_sizes(const dd_batch *b, dd_sizes *out)
{
    if (!b || !out) return fail(DD_ERR_INVALID, "null argument");
    if (check_offset_arrays(b)) return DD_ERR_INVALID;
    memset(out, 0, sizeof(*out));
    const int W = b->n_windows;
    out->n_haps = b->win_hap_off[W];
    out->n_reads = b->win_read_off[W];
    if (b->win_hap_off[0] != 0 || b->win_read_off[0] != 0 || b->hap_seq_off[0] != 0 || b->read_seq_off[0] != 0)
        return fail(DD_ERR_INVALID, "offset arrays must start at 0");
    for (int64_t h = 0; h < out->n_haps; h++) {
        int len = b->hap_seq_off[h + 1] - b->hap_seq_off[h];
        if (len < 0) return fail(DD_ERR_INVALID, "hap_seq_off not monotone");
        if (len > out->max_hap_len) out->max_hap_len = len;
    }
    for (int64_t r = 0; r < out->n_reads; r++) {
        int len = b->read_seq_off[r + 1] - b->read_seq_off[r];
        if (len < 0) return fail(DD_ERR_INVALID, "read_seq_off not monotone");
        if (len > out->max_read_len) out->max_read_len = len;
    }
    out->hap_bases = b->hap_seq_off[out->n_haps];
    out->read_bases = b->read_seq_off[out->n_reads];
    for (int w = 0; w < W; w++) {
        int64_t H = b->win_hap_off[w + 1] - b->win_hap_off[w];
        int64_t R = b->win_read_off[w + 1] - b->win_read_off[w];
        if (H < 0 || R < 0) return fail(DD_ERR_INVALID, "window offsets not monotone");
        int64_t SL = b->read_seq_off[b->win_read_off[w + 1]] - b->read_seq_off[b->win_read_off[w]];
        int64_t SH = b->hap_seq_off[b->win_hap_off[w + 1]] - b->hap_seq_off[b->win_hap_off[w]];
        int64_t nv = b->hap_var_off ? (b->hap_var_off[b->win_hap_off[w + 1]] - b->hap_var_off[b->win_hap_off[w]]) : 0;
        out->n_pairs += H * R;
        out->hpos_len += H * SL;
        out->var_cov_len += nv * R;
        out->cells += SH * SL;
    }
    return DD_SUCCESS;
}

int dd_screen_windows(const dd_batch *b, uint8_t *win_skip, int32_t max_len_out[2])
{
    if (!b || !win_skip) return fail(DD_ERR_INVALID, "null argument");
    if (check_offset_arrays(b)) return DD_ERR_INVALID;
    uint8_t lut[256];
    const int left = assign_symbols(b, lut);
    if (left < 0) return left;
    return screen_windows(b, win_skip, max_len_out, lut, left > 0);
}

int dd_screen_windows_ex(const dd_params *p, const dd_batch *b, uint32_t options, uint8_t *win_class, int32_t max_len_out[4])
{
    if (!b || !win_class) return fail(DD_ERR_INVALID, "null argument");
    if (check_offset_arrays(b)) return DD_ERR_INVALID;
    if (options & ~(DD_OPT_LONG_WINDOWS | DD_OPT_LONG_WINDOWS_FASTER | DD_OPT_WIDE_DELETIONS)) return fail(DD_ERR_INVALID, "unknown option bits");
    if ((options & DD_OPT_LONG_WINDOWS) && (options & DD_OPT_LONG_WINDOWS_FASTER))
        return fail(DD_ERR_INVALID, "DD_OPT_LONG_WINDOWS and DD_OPT_LONG_WINDOWS_FASTER class the windows for different models: one at a time");
    if ((options & DD_OPT_WIDE_DELETIONS) && !(options & DD_OPT_LONG_WINDOWS))      // (the --faster model's classes do not depend on the parameters)
        return fail(DD_ERR_INVALID, "DD_OPT_WIDE_DELETIONS needs DD_OPT_LONG_WINDOWS (the wide build is the long-window kernel's)");
    if (options) {
        const int rc = check_params(p, options);
        if (rc) return rc;
    }
    uint8_t lut[256];
    const int left = assign_symbols(b, lut);
    if (left < 0) return left;
    return screen_windows_ex(p, b, options, win_class, max_len_out, lut, left > 0);
}

int dd_batch_offsets(const dd_batch *b, int64_t *win_pair_off, int64_t *win_hpos_off, int64_t *win_varcov_off)
{
    if (!b) return fail(DD_ERR_INVALID, "null batch");
    int64_t p = 0, hp = 0, vc = 0;
    for (int w = 0; w < b->n_windows; w++) {
        if (win_pair_off) win_pair_off[w] = p;
        if (win_hpos_off) win_hpos_off[w] = hp;
        if (win_varcov_off) win_varcov_off[w] = vc;
        int64_t H = b->win_hap_off[w + 1] - b->win_hap_off[w];
        int64_t R = b->win_read_off[w + 1] - b->win_read_off[w];
        int64_t SL = b->read_seq_off[b->win_read_off[w + 1]] - b->read_seq_off[b->win_read_off[w]];
        int64_t nv = b->hap_var_off ? (b->hap_var_off[b->win_hap_off[w + 1]] - b->hap_var_off[b->win_hap_off[w]]) : 0;
        p += H * R; hp += H * SL; vc += nv * R;
    }
    if (win_pair_off) win_pair_off[b->n_windows] = p;
    if (win_hpos_off) win_hpos_off[b->n_windows] = hp;
    if (win_varcov_off) win_varcov_off[b->n_windows] = vc;
    return DD_SUCCESS;
}

int dd_build_index(const dd_batch *b, int32_t *hap_window, int64_t *win_pair_off, int64_t *win_hpos_off, int64_t *win_varcov_off)
{
    int rc = dd_batch_offsets(b, win_pair_off, win_hpos_off, win_varcov_off);
    if (rc) return rc;
    if (hap_window)
        for (int w = 0; w < b->n_windows; w++)
            for (int h = b->win_hap_off[w]; h < b->win_hap_off[w + 1]; h++) hap_window[h] = w;
    return DD_SUCCESS;
}

int dd_build_library_tables(const dd_batch *b, double *logprob_out, double *log95_out)
{
    if (!b || !logprob_out || !log95_out) return fail(DD_ERR_INVALID, "null argument");
    if (b->n_libs < 1 || b->n_libs > 256 || !b->lib_off || !b->lib_prob || !b->lib_p95)
        return fail(DD_ERR_INVALID, "mapUnmappedReads needs 1..256 libraries (lib_off, lib_prob, lib_p95)");
    if (b->lib_off[0] != 0) return fail(DD_ERR_INVALID, "lib_off[0] must be 0");
    for (int i = 0; i < b->n_libs; i++) {
        if (b->lib_off[i + 1] - b->lib_off[i] < 1) return fail(DD_ERR_INVALID, "empty library table");
        if (!(b->lib_p95[i] > 0.0)) return fail(DD_ERR_INVALID, "library probabilities must be positive");
        log95_out[i] = log(b->lib_p95[i]);                                   // ObservationModelFB.cpp:289
    }
    for (int i = 0; i < b->lib_off[b->n_libs]; i++) {
        if (!(b->lib_prob[i] > 0.0)) return fail(DD_ERR_INVALID, "library probabilities must be positive");
        logprob_out[i] = log(b->lib_prob[i]);                                // :285, :287
    }
    return DD_SUCCESS;
}

int dd_build_symbol_lut(const dd_batch *b, uint8_t *out)
{
    const int left = assign_symbols(b, out);
    return left < 0 ? left : DD_SUCCESS;        // bytes left without an id: their windows are dd_screen_windows' business
}

int dd_build_tables(const dd_params *p, const double *qual_table, int n_qual, const double *mapq_table, int n_mapq, double *out)
{
    return build_tables(p, qual_table, n_qual, mapq_table, n_mapq, out, 0);
}
int dd_build_tables_ex(const dd_params *p, const double *qual_table, int n_qual, const double *mapq_table, int n_mapq, double *out, uint32_t options)
{
    if (options & ~DD_OPT_WIDE_DELETIONS) return fail(DD_ERR_INVALID, "dd_build_tables_ex: unknown option bits (0 or DD_OPT_WIDE_DELETIONS)");
    return build_tables(p, qual_table, n_qual, mapq_table, n_mapq, out, options);
}
} // extern "C"
// the tables do not depend on maxLengthDel: options only decide which values of it pass the parameter check
int ddh::build_tables(const dd_params *p, const double *qual_table, int n_qual, const double *mapq_table, int n_mapq, double *out, uint32_t options)
{
    int rc = check_params(p, options);
    if (rc) return rc;
    if (n_qual < 0 || n_qual > DD_MAX_QUAL_TABLE || n_mapq < 0 || n_mapq > DD_MAX_QUAL_TABLE)
        return fail(DD_ERR_INVALID, "quality table larger than 256 entries");
    for (int i = 0; i < DD_TABLE_DOUBLES; i++) out[i] = 0.0;
    // ObservationModelFBMaxErr::setupTransitionProbs — reference ObservationModelFB.cpp:1643-1667
    const double logpInsgIns = -.5;
    const double logpInsgNoIns = log(p->pError);
    out[TC_LLL] = log(1.0 - p->pFirstgLO);
    out[TC_LFL] = log(p->pFirstgLO);
    out[TC_II] = logpInsgIns;
    out[TC_NI] = log(1.0 - exp(logpInsgIns));
    out[TC_IN] = logpInsgNoIns;
    out[TC_NN] = log(1 - p->pError);
    out[TC_EDEF] = log(1e-5);           // :1678
    out[TC_NDEF] = log(1 - 1e-5);       // :1679
    out[TC_BQT] = p->checkBaseQualThreshold;
    // emissions — setupReadObservationPotentials, reference ObservationModelFB.cpp:226-234
    for (int i = 0; i < n_qual; i++) {
        const double rq = qual_table[i];
        const double pr = rq * (1.0 - p->pMut);
        out[T_QUAL + 4 * i + 0] = log(.25 + .75 * pr);
        out[T_QUAL + 4 * i + 1] = log(.75 + 1e-10 - .75 * pr);
        out[T_QUAL + 4 * i + 2] = log10(1.0 - rq);      // mLogBQ term, :1406
        out[T_QUAL + 4 * i + 3] = rq;
    }
    // bMid prior — computeBMidPrior, reference ObservationModelFB.cpp:268-303 with pinsert == 0
    for (int i = -1; i < n_mapq; i++) {
        const double mapQual = (i < 0) ? (1.0 - 1e-10) : mapq_table[i];   // i<0: the "HMQ" prior of :1093
        double mq = 1.0 - mapQual;
        if (-10.0 * log10(mq) > p->mapQualThreshold) mq = pow(10.0, -p->mapQualThreshold / 10.0);
        const double pOffFirst = mq;
        const double pinsert = 0.0;
        double *dst = (i < 0) ? &out[TC_HMQ] : &out[T_MAPQ + 4 * i];
        for (int k = 0; k < 2; k++) {
            const double logpIns = (k == 1) ? logpInsgNoIns : log(1.0 - exp(logpInsgNoIns));
            dst[0 + k] = log(pOffFirst) + logpIns + pinsert;          // prior[i*numS+0]
            dst[2 + k] = pinsert + log((1.0 - pOffFirst)) + logpIns;  // prior[i*numS+x], 1<=x<=hapSize
        }
    }
    // insert-size prior path (mapUnmappedReads): the separate terms of computeBMidPrior — :272-276, :296-303
    out[TC_PINS + 0] = log(1.0 - exp(logpInsgNoIns));
    for (int i = -1; i < n_mapq; i++) {
        const double mapQual = (i < 0) ? (1.0 - 1e-10) : mapq_table[i];
        double mq = 1.0 - mapQual;
        if (-10.0 * log10(mq) > p->mapQualThreshold) mq = pow(10.0, -p->mapQualThreshold / 10.0);
        double *dst = (i < 0) ? &out[TC_PINS + 1] : &out[T_MAPQ2 + 2 * i];
        dst[0] = log(mq);
        dst[1] = log((1.0 - mq));
    }
    // --faster model: ObservationModelS::setupReadLikelihoods / SStateHMM constants — reference Faster.cpp:117-124, :300-352
    out[TC_FAST + 0] = log(1.0 - p->pError);
    out[TC_FAST + 1] = log(p->pError);
    out[TC_FAST + 2] = log(1 - exp(-0.25));
    out[TC_FAST + 3] = log(1.0 - 1e-10);
    out[TC_FAST + 4] = log(1e-10);
    for (int i = 0; i < n_mapq; i++) {
        double mq = 1.0 - mapq_table[i];
        if (-10.0 * log10(mq) > p->capMapQualFast) mq = pow(10.0, -p->capMapQualFast / 10.0);
        out[T_MAPQF + 2 * i] = log(1.0 - mq);
        out[T_MAPQF + 2 * i + 1] = log(mq);
    }
    // homopolymer indel-error logs — reference ObservationModelFB.cpp:1683-1703
    for (int len = 0; len < DD_HP_TABLE; len++) {
        const double perr = hp_error(len < 1 ? 1 : len);
        out[T_HP + 2 * len] = log(perr);
        out[T_HP + 2 * len + 1] = log(1.0 - perr);
    }
    return T_END;
}
extern "C" {

int dd_build_length_classes(const dd_batch *b, const uint8_t *win_skip, const dd_params *p, int32_t *hap_class_list, dd_length_classes *out)
{
    if (!b || !hap_class_list || !out) return fail(DD_ERR_INVALID, "null argument");
    return build_launch_classes(b, win_skip, p, hap_class_list, out);
}

// ---------------- several devices of one process ----------------
int dd_partition_windows(const dd_batch *b, int n_parts, int32_t *bounds)
{
    if (!b || !bounds || n_parts < 1) return fail(DD_ERR_INVALID, "null argument");
    if (check_offset_arrays(b)) return DD_ERR_INVALID;
    const int W = b->n_windows;
    std::vector<double> cum((size_t)W + 1, 0.0);          // cells before window w (exact in a double far beyond any batch)
    for (int w = 0; w < W; w++) {
        const int64_t SH = (int64_t)b->hap_seq_off[b->win_hap_off[w + 1]] - b->hap_seq_off[b->win_hap_off[w]];
        const int64_t SL = (int64_t)b->read_seq_off[b->win_read_off[w + 1]] - b->read_seq_off[b->win_read_off[w]];
        cum[(size_t)w + 1] = cum[(size_t)w] + (double)SH * (double)SL;
    }
    bounds[0] = 0;
    for (int i = 1; i < n_parts; i++) {
        // first boundary whose prefix reaches i/n of the work, moved one window back when that lands closer
        const double target = cum[(size_t)W] * (double)i / (double)n_parts;
        int w = (int)(std::lower_bound(cum.begin(), cum.end(), target) - cum.begin());
        if (w > 0 && target - cum[(size_t)w - 1] < cum[(size_t)w] - target) w--;
        if (w < bounds[i - 1]) w = bounds[i - 1];
        if (w > W) w = W;
        bounds[i] = w;
    }
    bounds[n_parts] = W;
    return DD_SUCCESS;
}

int dd_pair_sum_offsets(const dd_batch *b, int64_t *win_hh_off)
{
    if (!b || !win_hh_off) return fail(DD_ERR_INVALID, "null argument");
    int64_t o = 0;
    for (int w = 0; w < b->n_windows; w++) {
        win_hh_off[w] = o;
        const int64_t H = b->win_hap_off[w + 1] - b->win_hap_off[w];
        o += H * H;
    }
    win_hh_off[b->n_windows] = o;
    return DD_SUCCESS;
}
} // extern "C"
