// plan.cpp — the launch planner of the C ABI: lane tilings, LDS carve-up, occupancy, workgroup sizes and read splits, and the plans of the
// two long-window paths.  Pure host arithmetic: nothing here calls the HIP runtime.
#include "capi_internal.h"

namespace ddh {
using ddc::up16;

// Lane tilings, by haplotype length.  numS = Hs + 2 states go over the 64 lanes of a wavefront, K positions per lane (every K = 1..12 is
// instantiated, so no shape pays for more than 63 positions it does not have) — or, round 4, over the 32 lanes of HALF a wavefront, two
// pairs side by side (G = 2), where 32 K is the tighter fit: 127..158 bp run as K = 5 halves (2.5 lane-positions per pair instead of 3),
// 63..94 bp as K = 3 halves (1.5 instead of 2), <= 30 bp as K = 1 halves (0.5 instead of 1).
// Measured against the whole-wavefront tilings (tools/tiling_sweep.py, profiles/r04/tiling_sweep*.jsonl; 8 x 200 reads of 100 bp): <= 30 bp
// x 1.8, 63..94 bp + 1-7 %, 127..158 bp + 14-18 % (+ 4-9 % in ragged batches whose reads differ in length inside a window: the two reads
// of a wavefront run the longer one's trip counts).  31..62 bp as K = 2 halves were level with K = 1 on a whole wavefront (its FOLD build)
// and 191..222 bp as K = 7 halves gained 4-10 % on uniform windows of 100-bp reads but LOST 26-33 % on ragged ones with 150-bp reads (their
// LDS rows leave a CU 6 wavefronts, profiles/r04/wide_sample_ab.jsonl): both classes stay on a whole wavefront (the 191..222-bp class keeps
// its own launch: K = 4 like its neighbour).
const HapClassDef kHapClasses[DD_N_HAP_CLASSES] = {
    {30, 2, 1}, {62, 1, 1}, {94, 2, 3}, {126, 1, 2}, {158, 2, 5}, {190, 1, 3}, {222, 1, 4}, {254, 1, 4},
    {318, 1, 5}, {382, 1, 6}, {446, 1, 7}, {510, 1, 8}, {574, 1, 9}, {638, 1, 10}, {702, 1, 11}, {DD_MAX_HAP_LEN, 1, 12}};
static bool half_wave_off() { return getenv("DD_NO_HALF") != nullptr; }   // A/B and tests: whole-wavefront tilings only
int hap_class_of(int hap_len)
{
    for (int c = 0; c < DD_N_HAP_CLASSES; c++)
        if (hap_len <= kHapClasses[c].bound) return c;
    return -1;
}
// tiling for a launch whose longest haplotype is max_hap_len: false if it is too long
bool pick_tiling(int max_hap_len, int Dt, int &G, int &K)
{
    const int c = hap_class_of(max_hap_len);
    if (c < 0) return false;
    G = kHapClasses[c].G; K = kHapClasses[c].K;
    // (the half tilings in use gain at the D = 6, 11 and 12 builds: 9-16 % at maxLengthDel 10 / 11; the D = 32 build exists for whole
    // wavefronts only, up to K = 9 — 574 bp — because a position's back-pointer takes 7 bits there)
    if (G > 1 && (half_wave_off() || Dt > 12)) { G = 1; K = (kHapClasses[c].bound + 2 + 63) / 64; }
    if (Dt > 12 && K > 9) return false;
    return true;
}

int pick_Dt(int D)
{
    // every build switches candidates y > D off with -inf constants, so a smaller D runs on the next larger build
    // (maxLengthDel 0..4 on the D=6 build: 2.4e11 -> 4.0e11 cells/s at configs[1]; 6..9 on the D=11 build)
    if (D <= 6) return 6;
    if (D <= 11) return 11;
    if (D <= 12) return 12;
    return 32;                                    // maxLengthDel 12..31: the one build for the values beyond the reference's defaults (5 / 10)
}

// bytes of a lane's packed back-pointer word: K*(CB+1) bits per read base (BtPack in hmm_kernel.hip)
static uint32_t bt_word_bytes(int K, int Dt)
{
    const uint32_t bits = (uint32_t)K * ((Dt <= 7) ? 4u : (Dt <= 15 ? 5u : 7u));
    return bits <= 8 ? 1 : bits <= 16 ? 2 : bits <= 32 ? 4 : 8;
}

// LDS carve-up for (K, Dt, Lmax); returns total dynamic LDS bytes per workgroup
size_t lds_layout(int K, int Dt, int Lmax, int n_qual, int waves, bool gbt, int G, ddk::KernelArgs &A)
{
    const uint32_t W = 64u / (uint32_t)G;        // lanes per pair
    const uint32_t NP = W * K;
    uint32_t o = 0;
    o = up16(NP + 16);
    A.lds_off_L = o;  o += 256;                  // byte -> symbol id table
    A.lds_off_E = o;  o += up16((NP + Dt + 2) * 8);
    A.lds_off_N = o;  o += up16((NP + Dt + 2) * 8);
    A.lds_off_Q = o;  o += up16((uint32_t)n_qual * 32);
    A.n_qual = n_qual;
    A.lds_off_C = o;  A.lds_off_Y = o;
    if ((gbt || G > 1) && (Dt > 7 || K >= 3)) {  // LEAN build: block-shared Inc constants + (y-1)*II (hmm_kernel.hip)
        if (Dt <= 12) o += up16((uint32_t)K * Dt * W * 8u);   // (the D = 32 build forms these constants on the fly)
        A.lds_off_Y = o;  o += up16((uint32_t)Dt * 8u);
    }
    A.lds_off_W = o;  o += 16;                   // the workgroup's work counter
    A.lds_off_S = o;
    if (G > 1) o += up16(DD_HALF_CHUNK * 6u);    // half-wave builds: sort keys (u32) + order (u16) of a chunk of the window's reads
    A.lds_shared_bytes = o;
    uint32_t wv = 0;
    A.lds_off_A = wv;   wv += up16((uint32_t)K * (W + 2u * (uint32_t)((Dt + K - 1) / K)) * 16u);   // K arrays of {value, emission} + pads
    A.lds_off_I = wv;   wv += up16((NP + 2) * 8);
    A.lds_off_rdE = wv; wv += up16(Lmax * 16);
    A.lds_off_rdC = wv; wv += up16(Lmax);
    A.lds_off_rdQ = wv; wv += up16(Lmax);
    A.lds_off_ms = wv;  wv += up16(Lmax * 2);
    A.lds_group_bytes = wv;                      // the rows above exist once per pair of the wavefront; the back-pointer tile is the wavefront's
    wv *= (uint32_t)G;
    A.lds_off_bt = wv;
    if (!gbt) wv += up16((uint32_t)Lmax * 64u * bt_word_bytes(K, Dt));   // GBT builds keep the back-pointer tile in HBM scratch
    A.lds_wave_bytes = wv;
    return (size_t)A.lds_shared_bytes + (size_t)waves * wv;
}

// waves per CU the register file allows for each K (kernel-resource-usage of the shipped builds)
static int reg_limited_waves_per_cu(int K, int Dt, bool gbt, int G = 1)
{
    (void)G;
    if (Dt > 12) return K <= 3 ? 12 : (K <= 6 ? 8 : 4);   // the D = 32 build keeps a lane's own positions only: 125-144 registers up to K = 3, <= 244 up to K = 6
    if (const char *e = getenv("DD_REG_WAVES")) { const int v = atoi(e); if (v >= 1 && v <= 16) return v; }   // A/B builds with another occupancy
    if (K <= 2) return (Dt <= 7 || gbt) ? 12 : 8;
    if (K == 3) return (gbt && Dt <= 7) ? 12 : ((gbt || Dt <= 7) ? 8 : 4);      // round 3: the D = 6 scratch build is held to 168 VGPRs (3 waves/SIMD)
    if (K == 4) return gbt ? 8 : 4;
    if (K == 5 || G == 2) return gbt ? 8 : 4;    // round 4: the K = 5 scratch build held to 2 waves per SIMD gains 34 % over 1 (profiles/r04/occupancy_ab.txt)
    return 4;
}

// bytes of one wavefront's region of the HBM scratch: its back-pointer tile + (K >= 3 or half-wave builds) the [2 K][64] doubles where
// beta[bMid] waits for the join (hmm_kernel.hip STASH)
size_t scratch_wave_bytes(int K, int Dt, int G, int max_read_len)
{
    const bool slim = G > 1 || K == 3 || K == 5 || (K == 4 && Dt <= 7);       // hmm_kernel.hip SLIM
    return (size_t)max_read_len * 64u * bt_word_bytes(K, Dt) + (slim ? (size_t)2 * K * 64 * 8 : 0);
}

// Most waves a CU keeps resident over workgroups of DD_WAVES .. 1 waves (the larger workgroup on a tie), `cap` at the most;
// lds_bytes(wv): dynamic LDS of a workgroup of wv waves.  best_wv: that workgroup size, 0 if none fits the CU's LDS.
template <class LdsBytes> static int most_waves_per_cu(LdsBytes lds_bytes, int cap, int &best_wv)
{
    int best = 0;
    best_wv = 0;
    for (int wv = DD_WAVES; wv >= 1; wv--) {
        const size_t l = lds_bytes(wv);
        if (l > kCuLdsBytes) continue;
        const int total = std::min((int)(kCuLdsBytes / l) * wv, cap);
        if (total > best) { best = total; best_wv = wv; }
    }
    return best;
}

int make_plan(const dd_params *p, int max_hap_len, int max_read_len, int n_qual, Plan &pl, ddk::KernelArgs &A)
{
    pl.Dt = pick_Dt(p->maxLengthDel + 1);
    if (!pick_tiling(max_hap_len, pl.Dt, pl.G, pl.K))
        return fail(DD_ERR_UNSUPPORTED, pl.Dt > 12 ? "haplotype longer than 574 bp with maxLengthDel > 11" : "haplotype too long");
    int best[2] = {0, 0}, bw[2] = {0, 0}, cap[2] = {0, 0};
    auto lds_of = [&](bool gbt) { return [&, gbt](int wv) { ddk::KernelArgs tmp = A; return lds_layout(pl.K, pl.Dt, max_read_len, n_qual, wv, gbt, pl.G, tmp); }; };
    for (int gbt = 0; gbt < 2; gbt++) {
        cap[gbt] = reg_limited_waves_per_cu(pl.K, pl.Dt, gbt != 0, pl.G);
        best[gbt] = most_waves_per_cu(lds_of(gbt != 0), cap[gbt], bw[gbt]);
    }
    if (pl.Dt > 12) best[0] = 0;                   // the D = 32 build keeps its back-pointers in the HBM scratch only
    if (best[0] == 0 && best[1] == 0)
        return fail(DD_ERR_UNSUPPORTED, "read length x haplotype length does not fit the LDS row buffers");
    // K = 3 / D = 6 scratch: the 3-waves-per-SIMD build only where LDS lets 12 waves stay (reads up to ~250 bp); beyond, the build
    // for 2 waves per SIMD (no spills) with the geometry that fills 8: 9 waves of the spilling build lost 9 % to it at 400-bp reads
    pl.two_waves = false;
    if (pl.G == 1 && pl.K == 3 && pl.Dt <= 7 && best[1] > 0 && best[1] < 12) {
        pl.two_waves = true;
        cap[1] = 8;
        best[1] = most_waves_per_cu(lds_of(true), cap[1], bw[1]);
    }
    // HBM scratch costs a coalesced row fetch per 8 traceback steps and (D=11) block-shared constants; the LDS tile
    // costs occupancy.  Measured over six shapes (tools/ab_point.py with DD_FORCE_GBT=0/1): the LDS build wins
    // whenever its tile still lets the CU hold as many waves as its registers allow, the scratch build wins
    // (5-80 %) once LDS caps it below that (tools/plan_check.py grid: at 10 of 12 waves the scratch build is already
    // 14 % ahead).
    // For K >= 3 the scratch build is also the register-lean one (block-shared constants) and wins at every
    // shape measured (+26 ... +41 % in round 2; +10 ... +30 % on the round-3 grid) — except K = 3 at D = 6 with reads short
    // enough (<= 90 bp) for the LDS tile to keep the 8 waves its registers allow: there the LDS build is 4-10 % ahead of the
    // scratch build (profiles/r03/plan_check.jsonl, k3_lds_vs_scratch.jsonl), so that case follows the K <= 2 rule.
    // Round 4 (profiles/r04/plan_check.jsonl): K = 4 at D = 6 with reads up to ~80 bp is 17-18 % faster on the LDS build too (at 100 bp it loses 20 %).
    // End of round 4 (profiles/r04/plan_check.jsonl): with the item counter on every multi-round launch the scratch builds gained 10-18 % and the LDS builds
    // 1 %, and the exceptions above lost: K = 4 / D = 6 with reads <= 80 bp ran 35-45 % BEHIND on the LDS build, K = 3 / D = 6 with short reads 4-12 %, and
    // K = 2 on the D = 11 build 5-8 % at every read length the LDS tile fits.  Now: scratch for every K >= 3 and for K = 2 above D = 7.
    const bool lean_only = pl.K >= 3 || (pl.K == 2 && pl.Dt > 7);
    pl.gbt = best[0] == 0 || (lean_only && best[1] > 0) || best[0] < cap[0];
    if (const char *f = getenv("DD_FORCE_GBT")) {                  // A/B only
        if (f[0] == '1' && best[1] > 0) pl.gbt = true;
        if (f[0] == '0' && best[0] > 0) pl.gbt = false;
    }
    pl.waves = bw[pl.gbt ? 1 : 0];
    pl.waves_per_cu = best[pl.gbt ? 1 : 0];
    pl.lds = lds_layout(pl.K, pl.Dt, max_read_len, n_qual, pl.waves, pl.gbt, pl.G, A);
    pl.grid_cap = 0;
    pl.scratch_bytes = 0;
    if (pl.gbt) {
        const int blocks_per_cu = (pl.waves_per_cu + pl.waves - 1) / pl.waves;
        pl.grid_cap = (unsigned)kCUs * (unsigned)blocks_per_cu;
        pl.scratch_bytes = (size_t)pl.grid_cap * pl.waves * scratch_wave_bytes(pl.K, pl.Dt, pl.G, max_read_len);
    }
    return DD_SUCCESS;
}

// the plan alone, for callers that launch nothing
static int plan_only(const dd_params *p, int max_hap_len, int max_read_len, int n_qual, Plan &pl)
{
    ddk::KernelArgs A;
    memset(&A, 0, sizeof(A));
    return make_plan(p, max_hap_len, max_read_len, n_qual, pl, A);
}

int lds_read_threshold(const dd_params *p, int max_hap_len, int n_qual)
{
    if (!p || check_params(p) != DD_SUCCESS) return 0;
    int lo = 0, hi = 160;                       // largest L in [1, 160] whose plan keeps the back-pointers in LDS (0: none)
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        Plan pl;
        if (plan_only(p, max_hap_len, mid, n_qual > 0 ? n_qual : 1, pl) == DD_SUCCESS && !pl.gbt) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Waves per workgroup for windows with `units` units of work per haplotype (reads for the main kernel, groups of pairs for
// the --faster one): a workgroup's waves take the units round-robin, so with few units some waves idle in the last round
// while the workgroup's LDS stays allocated.  Keep `maxw` unless a smaller workgroup uses its waves > 10 % better
// (tools/coverage_sweep.py: 2 reads per window ran at half the rate with 4-wave workgroups).
// per_cu: waves the build keeps on a CU — workgroups of w waves leave per_cu % w of them unused (three-wave workgroups of a build
// held to 8 waves: 6 resident; the --faster kernel ran 10-read windows at 3.7e11 instead of 4.6e11 that way)
int waves_for_reads(int64_t units, int maxw, int per_cu)
{
    if (units < 1) units = 1;
    if (per_cu < maxw) per_cu = maxw;
    auto use = [&](int w) {
        return (double)units / (double)(((units + w - 1) / w) * w) * (double)((per_cu / w) * w) / (double)per_cu;
    };
    int best = maxw;
    double bestu = use(maxw);
    for (int w = maxw - 1; w >= 1; w--) {
        const double u = use(w);
        if (u > bestu * 1.10) { best = w; bestu = u; }
    }
    return best;
}

// Read split of a haplotype over workgroups.  One workgroup per haplotype is the cheapest (the per-haplotype setup is done
// once), but a small batch has too few haplotypes to fill the chip, a split that leaves the workgroup's `waves` waves a
// ragged number of rounds wastes wave slots (tools/batch_size_sweep.py), and a grid that is only a few times what the chip
// holds at once (`resident` workgroups) ends with a partly filled last round.  Among the splits from the one that yields
// `min_blocks` workgroups up to 8 x that, take the one with the best product of wave-slot use, round fill and setup
// amortisation (the per-haplotype tables cost about a quarter of one read's work per wave); within 1 % the smaller split
// wins.  Measured against the rule without the round term (DD_SPLIT_NO_ROUNDS=1, profiles/r03/split_ab.txt): 128 windows
// +4.6 %, 512 windows +1.8 %, the other sizes within 0.5 % — workgroups do not finish in lock step, so the rounds matter
// less than the count suggests.  resident == 0: the rounds are not modelled (the --faster kernel's callers).
int64_t pick_split(int64_t n_haps, int64_t units, int waves, int64_t min_blocks, int64_t resident)
{
    if (units < 1) units = 1;
    if (n_haps < 1) n_haps = 1;
    const int64_t max_split = (units + waves - 1) / waves;
    int64_t need = (min_blocks + n_haps - 1) / n_haps;
    if (need < 1) need = 1;
    if (need > max_split) need = max_split;
    if (resident <= 0) {
        int64_t best = need;
        double bestu = -1.0;
        for (int64_t sp = need; sp <= max_split; sp++) {
            const int64_t slots = sp * waves;
            const double u = (double)units / (double)(slots * ((units + slots - 1) / slots));
            if (u >= 0.9) return sp;
            if (u > bestu) { bestu = u; best = sp; }
        }
        return best;
    }
    int64_t best = need;
    double beste = -1.0;
    const int64_t last = std::min<int64_t>(max_split, need * 8);
    for (int64_t sp = need; sp <= last; sp++) {
        const int64_t slots = sp * waves;
        const double per_wave = (double)((units + slots - 1) / slots);          // reads of the busiest wave: the workgroup's duration
        const double use = (double)units / ((double)slots * per_wave);
        const int64_t n = n_haps * sp;
        const double fill = (double)n / (double)(((n + resident - 1) / resident) * resident);
        const double e = use * fill * per_wave / (per_wave + 0.25);
        if (e > beste * 1.01) { beste = e; best = sp; }
    }
    return best;
}

// workgroups of `waves` waves and `lds` bytes the chip holds at once, for a build that keeps waves_per_cu waves on a CU
int64_t resident_workgroups(size_t lds, int waves_per_cu, int waves)
{
    return kCUs * (int64_t)std::max(1, std::min((int)(kCuLdsBytes / (lds ? lds : 1)), waves_per_cu / waves));
}

// --faster model LDS: block-shared haplotype index + per-pair areas (layout in faster_kernel.hip's header)
size_t lds_layout_fast(int max_hap_len, int max_read_len, int n_qual, int &waves, int &groups, ddk::KernelArgs &A)
{
    uint32_t off = 0;
    A.lds_off_E = off; off = up16(off + 16u * (uint32_t)(n_qual > 0 ? n_qual : 1));
    A.lds_off_N = off; off = up16(off + (uint32_t)max_hap_len);
    A.lds_off_Q = off; off = up16(off + 2u * 257u);
    A.lds_off_C = off; off = up16(off + 2u * (uint32_t)max_hap_len);
    A.lds_off_Y = off; off = up16(off + 4u * 256u);
    A.lds_off_rdE = off; off = up16(off + 6u * 256u);          // FAST_CHUNK sort keys (u32) + ranks (u16)
    A.lds_shared_bytes = off;
    uint32_t po = 0;
    A.lds_off_A = po;   po = up16(po + 4u * (uint32_t)((max_hap_len + max_read_len + 1) / 2 + 1));
    A.lds_off_rdC = po; po = up16(po + 2u * (uint32_t)max_read_len);
    A.lds_off_bt = po;  po = up16(po + 16u * (uint32_t)max_read_len);
    A.lds_off_ms = A.lds_off_A;                  // the state path reuses the histogram bytes
    A.lds_off_I = po;   po = up16(po + 256u);
    A.lds_off_rdQ = po; po = up16(po + 64u);
    A.lds_wave_bytes = po;                       // bytes per PAIR area
    const size_t cap = kCuLdsBytes;
    // pair areas per wavefront: one per concurrent pair, plus a dummy for the idle 16-lane groups when fewer than 4 fit
    auto areas = [](int gq) { return gq < 4 ? gq + 1 : 4; };
    groups = 4;
    if (const char *e = getenv("DD_FAST_GROUPS")) {             // tests: exercise the fewer-pairs-per-wavefront geometry
        const int gq = atoi(e);
        if (gq == 1 || gq == 2) groups = gq;
    }
    while (groups > 1 && (size_t)off + (size_t)areas(groups) * po > cap) groups >>= 1;
    // waves per workgroup: whatever keeps the most wavefronts resident per CU (ties: more waves share one haplotype index)
    most_waves_per_cu([&](int wv) { return (size_t)off + (size_t)wv * areas(groups) * po; }, 8, waves);   // (8: the kernel is built for 2 waves per SIMD)
    if (waves < 1) waves = 1;
    if (const char *e = getenv("DD_FAST_WAVES")) {              // A/B only
        const int wv = atoi(e);
        if (wv >= 1 && wv <= DD_WAVES && (size_t)off + (size_t)wv * areas(groups) * po <= cap) waves = wv;
    }
    return (size_t)off + (size_t)waves * areas(groups) * po;
}

// header + window list + prefix list of a long workspace (kernel_common.h): where the prefix list and the tiles start
static uint64_t al256(uint64_t v) { return (v + 255u) & ~(uint64_t)255u; }
static void long_list_layout(int n_windows, uint64_t &off_prefix, uint64_t &off_tiles)
{
    off_prefix = al256(DD_LWS_HEADER + 4 * (uint64_t)std::max(n_windows, 1));
    off_tiles = al256(off_prefix + 8 * (uint64_t)(std::max(n_windows, 0) + 1));
}

// ---------------- long windows of the main model (long_kernel.hip) ----------------
// Plan of a long launch: K states per thread (numS <= 256 K, K = 1, 2, 4, 8, 16), LDS, and the persistent grid: the chip's resident
// workgroups (LDS- and register-limited: 2 per CU, 1 at K = 16), shrunk so that header + lists + one back-pointer tile per workgroup stay
// within DD_LONG_WS_BUDGET.
int long_plan(int n_windows, int max_hap_len, int max_read_len, int n_qual, LongPlan &lp, ddl::LongArgs &A)
{
    if (max_hap_len < 1 || max_hap_len > DD_LONG_MAX_HAP_LEN) return fail(DD_ERR_UNSUPPORTED, "long path: haplotype length outside [1,4094]");
    if (max_read_len < 1 || max_read_len > DD_LONG_MAX_READ_LEN) return fail(DD_ERR_UNSUPPORTED, "long path: read length outside [1,4096]");
    const int numS = max_hap_len + 2;
    lp.K = 1;
    while (DD_LONG_THREADS * lp.K < numS) lp.K *= 2;
    A.n_qual = n_qual;
    lp.lds = ddl::long_lds_layout(lp.K, max_read_len, A);
    if (lp.lds + 64 > kCuLdsBytes) return fail(DD_ERR_UNSUPPORTED, "long path: LDS layout too large");
    const unsigned per_cu = std::max(1u, std::min(lp.K >= 16 ? 1u : 2u, (unsigned)((kCuLdsBytes) / (lp.lds + 64))));
    long_list_layout(n_windows, lp.off_lpoff, lp.off_tiles);
    lp.stash_off = al256((uint64_t)max_read_len * DD_LONG_THREADS * lp.K);
    lp.tile_bytes = lp.stash_off + 16 * (uint64_t)DD_LONG_THREADS * lp.K;
    uint64_t grid = (uint64_t)kCUs * per_cu;
    const uint64_t fit = DD_LONG_WS_BUDGET > lp.off_tiles ? (DD_LONG_WS_BUDGET - lp.off_tiles) / lp.tile_bytes : 0;
    if (grid > fit) grid = fit;
    if (grid < 1) grid = 1;
    lp.grid = (unsigned)grid;
    lp.ws_bytes = lp.off_tiles + grid * lp.tile_bytes;
    return DD_SUCCESS;
}

// ---------------- long windows of the --faster model (faster_long_kernel.hip) ----------------
// Plan of a launch: LDS for the shape, and the persistent grid: the chip's resident workgroups (LDS-limited, at most 2 per CU: the kernel is
// built for 2 waves per SIMD), no more than the batch can have 16-pair items, shrunk so that header + lists + 16 tiles per workgroup stay
// within DD_FASTER_LONG_WS_BUDGET.
int fl_plan(const dd_device_batch *b, FLPlan &fp, ddf::FLArgs &A)
{
    const int mh = b->long_max_hap_len, mr = b->long_max_read_len;
    if (mh < 1 || mh > DD_LONG_MAX_HAP_LEN) return fail(DD_ERR_UNSUPPORTED, "--faster long path: haplotype length outside [1,4094]");
    if (mr < 1 || mr > DD_LONG_MAX_READ_LEN) return fail(DD_ERR_UNSUPPORTED, "--faster long path: read length outside [1,4096]");
    A.n_qual = b->n_qual;
    A.max_hap_len = mh; A.max_read_len = mr;
    fp.lds = ddf::fl_lds_layout(mh, mr, A);
    if (fp.lds + 64 > kCuLdsBytes) return fail(DD_ERR_UNSUPPORTED, "--faster long path: LDS layout too large");
    const unsigned per_cu = std::max(1u, std::min(2u, (unsigned)((kCuLdsBytes) / (fp.lds + 64))));
    long_list_layout(b->n_windows, fp.off_ioff, fp.off_tiles);
    const uint64_t wg_bytes = DD_FL_PAIRS * ddf::fl_tile_layout(mh, mr, A);
    uint64_t grid = (uint64_t)kCUs * per_cu;
    const uint64_t items = (uint64_t)std::max(b->n_haps, 0) * (((uint64_t)std::max(b->n_reads, 0) + DD_FL_PAIRS - 1) / DD_FL_PAIRS);
    if (grid > items) grid = items;
    const uint64_t fit = DD_FASTER_LONG_WS_BUDGET > fp.off_tiles ? (DD_FASTER_LONG_WS_BUDGET - fp.off_tiles) / wg_bytes : 0;
    if (grid > fit) grid = fit;
    if (grid < 1) grid = 1;
    fp.grid = (unsigned)grid;
    fp.ws_bytes = fp.off_tiles + grid * wg_bytes;
    A.off_ioff = fp.off_ioff; A.off_tiles = fp.off_tiles; A.grid = (int32_t)grid;
    return DD_SUCCESS;
}
} // namespace ddh
using namespace ddh;
extern "C" {
size_t dd_workspace_bytes(const dd_params *p, const dd_device_batch *b)
{
    if (!p || !b || check_params(p) != DD_SUCCESS) return 0;
    if (b->max_hap_len < 1 || b->max_read_len < 1) return 0;
    Plan pl;
    if (plan_only(p, b->max_hap_len, b->max_read_len, b->n_qual, pl) != DD_SUCCESS) return 0;
    size_t bytes = pl.scratch_bytes;
    if (b->classes && b->hap_class_list)          // per-class launches: the largest scratch any of them needs
        for (int i = 0; i < b->classes->n_launches; i++)
            if (plan_only(p, b->classes->launch[i].max_hap_len, b->classes->launch[i].max_read_len, b->n_qual, pl) == DD_SUCCESS)
                bytes = std::max(bytes, pl.scratch_bytes);
    return bytes + DD_WS_HEADER;                  // the work counter of the ragged launches in front of the back-pointer tiles
}

size_t dd_workspace_bytes_long(const dd_params *p, const dd_device_batch *b)
{
    (void)p;
    if (!b || b->long_max_hap_len <= 0 || b->long_max_read_len <= 0) return 0;
    ddl::LongArgs A;
    memset(&A, 0, sizeof(A));
    LongPlan lp;
    if (long_plan(b->n_windows, b->long_max_hap_len, b->long_max_read_len, b->n_qual, lp, A)) return 0;
    return (size_t)lp.ws_bytes;
}

size_t dd_workspace_bytes_faster_long(const dd_params *p, const dd_device_batch *b)
{
    (void)p;
    if (!b || b->long_max_hap_len <= 0 || b->long_max_read_len <= 0) return 0;
    ddf::FLArgs A;
    memset(&A, 0, sizeof(A));
    FLPlan fp;
    if (fl_plan(b, fp, A)) return 0;
    return (size_t)fp.ws_bytes;
}

int dd_plan_info(const dd_params *p, int max_hap_len, int max_read_len, int n_qual, int avg_reads, int n_haps, int32_t out[10])
{
    int rc = check_params(p);
    if (rc) return rc;
    if (!out) return fail(DD_ERR_INVALID, "null argument");
    if (max_hap_len < 1 || max_hap_len > DD_MAX_HAP_LEN) return fail(DD_ERR_UNSUPPORTED, "haplotype length outside [1,766]");
    if (max_read_len < 1 || max_read_len > DD_MAX_READ_LEN) return fail(DD_ERR_UNSUPPORTED, "read length outside [1,1024]");
    Plan pl;
    ddk::KernelArgs A;
    memset(&A, 0, sizeof(A));
    if ((rc = make_plan(p, max_hap_len, max_read_len, n_qual, pl, A))) return rc;
    const int waves = waves_for_reads((avg_reads + pl.G - 1) / pl.G, pl.waves, pl.waves_per_cu);
    out[8] = pl.G; out[9] = 0;
    avg_reads = (avg_reads + pl.G - 1) / pl.G;   // units of work per haplotype: a wavefront takes G reads at a time
    out[0] = pl.K; out[1] = pl.Dt; out[2] = pl.gbt ? 1 : 0; out[3] = waves;
    out[5] = (int32_t)lds_layout(pl.K, pl.Dt, max_read_len, n_qual, waves, pl.gbt, pl.G, A);
    out[4] = (int32_t)pick_split(n_haps, avg_reads, waves, 4096, resident_workgroups((size_t)out[5], pl.waves_per_cu, waves));
    out[6] = (int32_t)((pl.scratch_bytes >> 10) & 0x7fffffff);
    out[7] = pl.waves_per_cu;
    return DD_SUCCESS;
}
} // extern "C"
