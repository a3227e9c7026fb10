// plan.cpp — the launch planner of the C ABI: lane tilings, LDS carve-up, occupancy, workgroup sizes and read splits; the whole shape of a
// main-model or --faster launch (shape_launch, shape_fast) and its three descriptions; the A/B switches (read_switches).  Pure host
// arithmetic: nothing here calls the HIP runtime or needs a kernel unit to link (the plans of the long-window paths are long_plan.cpp).
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
int hap_class_of(int hap_len)
{
    for (int c = 0; c < DD_N_HAP_CLASSES; c++)
        if (hap_len <= kHapClasses[c].bound) return c;
    return -1;
}
// tiling for a launch whose longest haplotype is max_hap_len: false if it is too long
bool pick_tiling(const Switches &sw, int max_hap_len, int Dt, int &G, int &K)
{
    const int c = hap_class_of(max_hap_len);
    if (c < 0) return false;
    G = kHapClasses[c].G; K = kHapClasses[c].K;
    // (the half tilings in use gain at the D = 6, 11 and 12 builds: 9-16 % at maxLengthDel 10 / 11; the D = 32 build exists for whole
    // wavefronts only, up to K = 9 — 574 bp — because a position's back-pointer takes 7 bits there)
    if (G > 1 && (sw.no_half || Dt > 12)) { G = 1; K = (kHapClasses[c].bound + 2 + 63) / 64; }
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
static size_t lds_layout(int K, int Dt, int Lmax, int n_qual, int waves, bool gbt, int G, ddk::KernelArgs &A)
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
static int reg_limited_waves_per_cu(const Switches &sw, int K, int Dt, bool gbt, int G = 1)
{
    (void)G;
    if (Dt > 12) return K <= 3 ? 12 : (K <= 6 ? 8 : 4);   // the D = 32 build keeps a lane's own positions only: 125-144 registers up to K = 3, <= 244 up to K = 6
    if (sw.reg_waves) return sw.reg_waves;      // A/B builds with another occupancy
    if (K <= 2) return (Dt <= 7 || gbt) ? 12 : 8;
    if (K == 3) return (gbt && Dt <= 7) ? 12 : ((gbt || Dt <= 7) ? 8 : 4);      // round 3: the D = 6 scratch build is held to 168 VGPRs (3 waves/SIMD)
    if (K == 4) return gbt ? 8 : 4;
    if (K == 5 || G == 2) return gbt ? 8 : 4;    // round 4: the K = 5 scratch build held to 2 waves per SIMD gains 34 % over 1 (profiles/r04/occupancy_ab.txt)
    return 4;
}

// bytes of one wavefront's region of the HBM scratch: its back-pointer tile + (K >= 3 or half-wave builds) the [2 K][64] doubles where
// beta[bMid] waits for the join (hmm_kernel.hip STASH)
static size_t scratch_wave_bytes(int K, int Dt, int G, int max_read_len)
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

static int make_plan(const Switches &sw, const dd_params *p, int max_hap_len, int max_read_len, int n_qual, Plan &pl, ddk::KernelArgs &A)
{
    pl.Dt = pick_Dt(p->maxLengthDel + 1);
    if (!pick_tiling(sw, max_hap_len, pl.Dt, pl.G, pl.K))
        return fail(DD_ERR_UNSUPPORTED, pl.Dt > 12 ? "haplotype longer than 574 bp with maxLengthDel > 11" : "haplotype too long");
    int best[2] = {0, 0}, bw[2] = {0, 0}, cap[2] = {0, 0};
    auto lds_of = [&](bool gbt) { return [&, gbt](int wv) { ddk::KernelArgs tmp = A; return lds_layout(pl.K, pl.Dt, max_read_len, n_qual, wv, gbt, pl.G, tmp); }; };
    for (int gbt = 0; gbt < 2; gbt++) {
        cap[gbt] = reg_limited_waves_per_cu(sw, pl.K, pl.Dt, gbt != 0, pl.G);
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
    if (sw.force_gbt == 1 && best[1] > 0) pl.gbt = true;          // A/B only
    if (sw.force_gbt == 0 && best[0] > 0) pl.gbt = false;
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
static int plan_only(const Switches &sw, const dd_params *p, int max_hap_len, int max_read_len, int n_qual, Plan &pl)
{
    ddk::KernelArgs A;
    memset(&A, 0, sizeof(A));
    return make_plan(sw, p, max_hap_len, max_read_len, n_qual, pl, A);
}

int lds_read_threshold(const Switches &sw, const dd_params *p, int max_hap_len, int n_qual)
{
    if (!p || check_params(p) != DD_SUCCESS) return 0;
    int lo = 0, hi = 160;                       // largest L in [1, 160] whose plan keeps the back-pointers in LDS (0: none)
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        Plan pl;
        if (plan_only(sw, p, max_hap_len, mid, n_qual > 0 ? n_qual : 1, pl) == DD_SUCCESS && !pl.gbt) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Waves per workgroup for windows with `units` units of work per haplotype (reads for the main kernel, groups of pairs for
// the --faster one): a workgroup's waves take the units round-robin, so with few units some waves idle in the last round
// while the workgroup's LDS stays allocated.  Keep `maxw` unless a smaller workgroup uses its waves > 10 % better
// (tools/coverage_sweep.py: 2 reads per window ran at half the rate with 4-wave workgroups).
// per_cu: waves the build keeps on a CU — workgroups of w waves leave per_cu % w of them unused (three-wave workgroups of a build
// held to 8 waves: 6 resident; the --faster kernel ran 10-read windows at 3.7e11 instead of 4.6e11 that way)
static int waves_for_reads(int64_t units, int maxw, int per_cu)
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
static int64_t pick_split(int64_t n_haps, int64_t units, int waves, int64_t min_blocks, int64_t resident = 0)
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
static int64_t resident_workgroups(size_t lds, int waves_per_cu, int waves)
{
    return kCUs * (int64_t)std::max(1, std::min((int)(kCuLdsBytes / (lds ? lds : 1)), waves_per_cu / waves));
}

// --faster model: LDS bytes of a workgroup of `waves` waves with `groups` pairs per wavefront, from the layout in A.  Pair areas per
// wavefront: one per concurrent pair, plus a dummy for the idle 16-lane groups when fewer than 4 fit.
static size_t fast_lds_bytes(const ddk::KernelArgs &A, int waves, int groups)
{
    return (size_t)A.lds_shared_bytes + (size_t)waves * (groups < 4 ? groups + 1 : 4) * A.lds_wave_bytes;
}

// --faster model LDS: block-shared haplotype index + per-pair areas (layout in faster_kernel.hip's header)
static size_t lds_layout_fast(const Switches &sw, int max_hap_len, int max_read_len, int n_qual, int &waves, int &groups, ddk::KernelArgs &A)
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
    groups = 4;
    if (sw.fast_groups) groups = sw.fast_groups;                // tests: exercise the fewer-pairs-per-wavefront geometry
    while (groups > 1 && fast_lds_bytes(A, 1, groups) > kCuLdsBytes) groups >>= 1;
    // waves per workgroup: whatever keeps the most wavefronts resident per CU (ties: more waves share one haplotype index)
    most_waves_per_cu([&](int wv) { return fast_lds_bytes(A, wv, groups); }, 8, waves);   // (8: the kernel is built for 2 waves per SIMD)
    if (waves < 1) waves = 1;
    if (sw.fast_waves && fast_lds_bytes(A, sw.fast_waves, groups) <= kCuLdsBytes) waves = sw.fast_waves;   // A/B only
    return fast_lds_bytes(A, waves, groups);
}

Switches read_switches()
{
    Switches sw;
    auto on = [](const char *name) { return getenv(name) != nullptr; };
    auto num = [](const char *name) { const char *e = getenv(name); return e ? atoi(e) : 0; };
    sw.no_half = on("DD_NO_HALF");
    if (const int v = num("DD_REG_WAVES"); v >= 1 && v <= 16) sw.reg_waves = v;
    if (const char *e = getenv("DD_FORCE_GBT")) sw.force_gbt = e[0] == '1' ? 1 : (e[0] == '0' ? 0 : -1);
    if (const int v = num("DD_FAST_GROUPS"); v == 1 || v == 2) sw.fast_groups = v;
    if (const int v = num("DD_FAST_WAVES"); v >= 1 && v <= DD_WAVES) sw.fast_waves = v;
    if (const char *e = getenv("DD_FAST_TARGET_BLOCKS")) { const long v = atol(e); if (v >= 1) sw.fast_target_blocks = v; }
    sw.always_ro = on("DD_ALWAYS_RO");
    if (const char *e = getenv("DD_TARGET_BLOCKS")) { const long v = atol(e); if (v >= 1) sw.target_blocks = v; }
    sw.split_no_rounds = on("DD_SPLIT_NO_ROUNDS");
    sw.uniform_split = on("DD_UNIFORM_SPLIT");
    if (const int v = num("DD_READS_PER_WAVE"); v >= 1) sw.reads_per_wave = v;
    if (const char *e = getenv("DD_DYNAMIC")) sw.dynamic = e[0] == '1' ? 1 : 0;
    sw.no_fold = on("DD_NO_FOLD");
    sw.no_promote = on("DD_NO_PROMOTE");
    if (const char *e = getenv("DD_LENGTH_CLASSES")) sw.one_read_class = !strcmp(e, "k");
    if (on("DD_READ_BOUND")) sw.read_bound = std::max(num("DD_READ_BOUND"), 0);
    return sw;
}

// The builds measured to gain from the fold (end states inside the generic candidate code, hmm_kernel.hip FOLD): K <= 2 at D build 6 with
// LDS back-pointers, K = 2 at D build 6 with scratch back-pointers, K = 2 at D build 11 with LDS back-pointers.  (Not build_launch_classes'
// "tilings that have a folded build": that one asks which haplotypes are worth a launch of their own.)
static bool launch_has_fold_build(const Plan &pl)
{
    return pl.gbt ? (pl.K == 2 && pl.Dt == 6) : ((pl.K <= 2 && pl.Dt == 6) || (pl.K == 2 && pl.Dt == 11));
}

int shape_launch(const Switches &sw, const LaunchAsk &ask, LaunchShape &s, ddk::KernelArgs &A)
{
    s = LaunchShape();
    const ClassDims *lc = ask.has_class ? &ask.cls : nullptr;
    const int cls_hap = lc ? lc->max_hap_len : ask.max_hap_len, cls_read = lc ? lc->max_read_len : ask.max_read_len;
    Plan &pl = s.pl;
    const int rc = make_plan(sw, ask.p, cls_hap, cls_read, ask.n_qual, pl, A);
    if (rc) return rc;
    const int K = pl.K, Dt = pl.Dt;
    s.waves = pl.waves;
    s.lds = pl.lds;
    // thin windows: a wavefront works on one read at a time, so a workgroup never needs more waves than the windows have
    // reads (tools/coverage_sweep.py: 2 reads per window ran at half the rate with idle waves in every workgroup)
    const int64_t avg_reads = (lc && lc->avg_window_reads > 0) ? lc->avg_window_reads : (ask.n_reads + ask.n_windows - 1) / (ask.n_windows > 0 ? ask.n_windows : 1);
    const int64_t units = (avg_reads + pl.G - 1) / pl.G;                       // a wavefront takes G reads at a time
    if (const int w2 = waves_for_reads(units, s.waves, pl.waves_per_cu); w2 != s.waves) {
        s.waves = w2;
        s.lds = lds_layout(K, Dt, cls_read, ask.n_qual, w2, pl.gbt, pl.G, A);
    }
    s.lds_wave_bytes = A.lds_wave_bytes;
    s.lds_shared_bytes = A.lds_shared_bytes;
    if (pl.gbt) {
        if (ask.workspace_bytes < pl.scratch_bytes + DD_WS_HEADER)
            return fail(DD_ERR_INVALID, "workspace too small for this shape: allocate dd_workspace_bytes() bytes");
        s.scratch_off = DD_WS_HEADER;
        s.bt_rows = cls_read;
        s.bt_wave_bytes = (uint32_t)scratch_wave_bytes(K, Dt, pl.G, cls_read);
    }
    int hap_begin = ask.hap_begin, hap_end = ask.hap_end;
    if (hap_end < 0) { hap_begin = 0; hap_end = ask.n_haps; }
    if (lc && lc->listed) { hap_begin = lc->list_begin; hap_end = lc->list_end; }   // positions in the class list
    s.n_haps = hap_end - hap_begin; s.max_hap = cls_hap; s.min_read = lc ? lc->min_read_len : 1; s.max_read = cls_read;
    // the split is chosen for the haplotypes THIS launch covers: a rare length class or a small window block must still
    // spread over the chip; enough workgroups to fill 256 CUs several times over (target_blocks), but keep >= 1 read per wave
    // resident: workgroups the chip holds at once (one-shot grids; a persistent GBT grid is capped to that number below anyway)
    int64_t resident = resident_workgroups(s.lds, pl.waves_per_cu, s.waves);
    if (sw.split_no_rounds) resident = 0;                                      // A/B only: the rule before round 3
    s.split = pick_split(s.n_haps, units, s.waves, sw.target_blocks, resident);
    // Ragged windows: `split` suits a window with the average number of reads; a haplotype whose window has more gets proportionally more
    // workgroups (the kernel derives its own count from reads_per_wave), so that a 400-read window among 100-read ones does not end the
    // launch with one workgroup still at work; when the spread is wide the work of a wavefront is also capped (DD_READS_PER_WAVE, A/B).
    const int max_reads = (lc && lc->max_window_reads > 0) ? lc->max_window_reads : ask.max_window_reads;
    if (max_reads > 0 && max_reads * 4 > avg_reads * 5 && !sw.uniform_split) {
        const int64_t max_units = (max_reads + pl.G - 1) / pl.G;
        const int64_t cap_rpw = sw.reads_per_wave ? sw.reads_per_wave : ((Dt > 7 || K >= 3) ? 24 : 12);
        const int64_t rpw = std::max<int64_t>(1, std::min((units + s.waves * s.split - 1) / (s.waves * s.split), cap_rpw));
        s.reads_per_wave = (int)rpw;
        s.split = std::max<int64_t>(1, (max_units + s.waves * rpw - 1) / (s.waves * rpw));
    }
    if ((int64_t)ask.n_haps * s.split > 0x7fffffffLL) return fail(DD_ERR_UNSUPPORTED, "batch too large for one launch");
    s.item_begin = (int32_t)(hap_begin * s.split);
    s.n_items = (int32_t)(hap_end * s.split);
    s.n_launch_items = s.grid = (int64_t)s.n_haps * s.split;
    if (s.grid <= 0) return DD_SUCCESS;
    if (pl.grid_cap)     // the scratch holds grid_cap x pl.waves back-pointer tiles; smaller workgroups (thin windows) may be more numerous
        s.grid = std::min(s.grid, (int64_t)pl.grid_cap * pl.waves / s.waves);
    // More items than the chip holds workgroups: a persistent grid that draws its items from a counter.  Built for the ragged launches (items that
    // differ 20-fold in work); at the end of round 4 it turned out to be worth as much on UNIFORM batches wherever the grid was persistent
    // already — every HBM-scratch build ran a fixed stride, and the items of a uniform batch still differ by their reads' bMid: 3.42 -> 3.85e11 cells/s
    // at 130 bp, 3.34 -> 3.88e11 at 80 bp, +10-18 % on every K >= 3 tiling (profiles/r04/item_counter_uniform_ab.txt) — and +0.1-1.5 % on the
    // one-shot LDS grids (the headline build: +0.9 %), whose XCD-contiguous numbering (one L2 per window's haplotypes) it gives up.
    // (Except: the chunks of the host-pointer path alternate between two streams, and a one-shot grid lets the next chunk's workgroups move in
    // while this one's drain; a chip-filling persistent grid holds its slots to the end — `dd_compute_likelihoods` with pageable pointers lost 7 %
    // that way, 23.7 -> 22.0 k windows/s at configs[1].  There the LDS builds keep their one-shot grids unless the batch is ragged.)
    const bool spread = s.reads_per_wave > 0 || (lc && lc->avg_read_len > 0 && lc->max_read_len * 4 > lc->avg_read_len * 5);
    const bool dynamic = sw.dynamic >= 0 ? sw.dynamic == 1 : (pl.gbt || spread || !ask.overlapping_chunks);   // DD_DYNAMIC=0: one-shot LDS grids, fixed stride on scratch builds
    if (dynamic && ask.workspace_bytes >= DD_WS_HEADER && resident > 0 && s.n_launch_items > resident) {
        s.use_counter = true;
        s.grid = std::min(s.grid, resident);
    }
    // the FOLD build needs every haplotype of this launch to leave position 64 K - 1 idle (numS <= 64 K - 1)
    s.fold = pl.G == 1 && launch_has_fold_build(pl) && 64 * K >= cls_hap + 3 && !sw.no_fold;
    s.occ = (pl.gbt && pl.two_waves) ? 2 : 0;
    s.build = (s.fold ? DD_BUILD_FOLD : 0) | (s.occ == 2 ? DD_BUILD_TWO_WAVES : 0) | (pl.G == 2 ? DD_BUILD_HALF : 0);
    return DD_SUCCESS;
}

int shape_fast(const Switches &sw, const LaunchAsk &ask, LaunchShape &s, ddk::KernelArgs &A)
{
    s = LaunchShape();
    s.faster = true;
    s.lds = lds_layout_fast(sw, ask.max_hap_len, ask.max_read_len, ask.n_qual, s.waves, s.groups, A);
    if (s.lds > kCuLdsBytes) return fail(DD_ERR_UNSUPPORTED, "shape exceeds the LDS tile of the --faster kernel");
    s.lds_wave_bytes = A.lds_wave_bytes;
    const int64_t avg_reads = (ask.n_reads + ask.n_windows - 1) / (ask.n_windows > 0 ? ask.n_windows : 1);
    const int64_t units = (avg_reads + s.groups - 1) / s.groups;
    // thin windows: no more wavefronts per workgroup than the windows have groups of `groups` reads
    if (const int w2 = waves_for_reads(units, s.waves, 8); w2 != s.waves) {
        s.waves = w2;
        s.lds = fast_lds_bytes(A, w2, s.groups);
    }
    int hap_begin = ask.hap_begin, hap_end = ask.hap_end;
    if (hap_end < 0) { hap_begin = 0; hap_end = ask.n_haps; }
    s.n_haps = hap_end - hap_begin;
    s.split = pick_split(s.n_haps, units, s.waves, sw.fast_target_blocks);
    if ((int64_t)ask.n_haps * s.split > 0x7fffffffLL) return fail(DD_ERR_UNSUPPORTED, "batch too large for one launch");
    s.item_begin = (int32_t)(hap_begin * s.split);
    s.n_items = (int32_t)(hap_end * s.split);
    s.n_launch_items = s.grid = (int64_t)s.n_haps * s.split;
    return DD_SUCCESS;
}

void shape_last_launch(const LaunchShape &s, int32_t out[8])
{   // K (--faster: pairs per wavefront), D build (+ 100: scratch back-pointers; --faster: 0), waves per workgroup, LDS bytes per workgroup, grid, read split,
    // LDS per wave, shared LDS
    const int32_t v[8] = {s.faster ? s.groups : s.pl.K, s.faster ? 0 : s.pl.Dt + (s.pl.gbt ? 100 : 0), s.waves, (int32_t)s.lds, (int32_t)s.grid,
                          (int32_t)s.split, (int32_t)s.lds_wave_bytes, (int32_t)s.lds_shared_bytes};
    memcpy(out, v, sizeof(v));
}

void shape_kernel_name(const LaunchShape &s, char *name, size_t size)
{   // the template instance as rocprofv3 prints it (inside "void ddk::...(ddk::KernelArgs)"); no launch yet: the main kernel's plain name
    if (s.faster) snprintf(name, size, "dd_faster_kernel");
    else if (s.pl.K > 0) snprintf(name, size, "dd_hmm_kernel<%d, %d, %s, %s, %d, %d>", s.pl.K, s.pl.Dt, s.pl.gbt ? "true" : "false", s.fold ? "true" : "false", s.occ, s.pl.G);
    else snprintf(name, size, "dd_hmm_kernel");
}

void shape_log_record(const LaunchShape &s, int32_t v[DD_LAUNCH_LOG_FIELDS])
{   // include/dindel_hmm.h dd_launch_log; field 15, the duration, is filled in when the log is read
    const int32_t r[DD_LAUNCH_LOG_FIELDS] = {s.pl.K, s.pl.G, s.pl.Dt, s.pl.gbt ? 1 : 0, s.fold ? 1 : 0, s.waves, (int32_t)s.lds, (int32_t)s.grid, (int32_t)s.split,
                                             s.n_haps, s.max_hap, s.min_read, s.max_read, s.pl.waves_per_cu, s.occ, -1, s.use_counter ? 1 : 0, s.reads_per_wave};
    memcpy(v, r, sizeof(r));
}
} // namespace ddh
using namespace ddh;
extern "C" {
size_t dd_workspace_bytes(const dd_params *p, const dd_device_batch *b)
{
    if (!p || !b || check_params(p) != DD_SUCCESS) return 0;
    if (b->max_hap_len < 1 || b->max_read_len < 1) return 0;
    const Switches sw = read_switches();
    Plan pl;
    if (plan_only(sw, p, b->max_hap_len, b->max_read_len, b->n_qual, pl) != DD_SUCCESS) return 0;
    size_t bytes = pl.scratch_bytes;
    if (b->classes && b->hap_class_list)          // per-class launches: the largest scratch any of them needs
        for (int i = 0; i < b->classes->n_launches; i++)
            if (plan_only(sw, p, b->classes->launch[i].max_hap_len, b->classes->launch[i].max_read_len, b->n_qual, pl) == DD_SUCCESS)
                bytes = std::max(bytes, pl.scratch_bytes);
    return bytes + DD_WS_HEADER;                  // the work counter of the ragged launches in front of the back-pointer tiles
}

int dd_plan_info(const dd_params *p, int max_hap_len, int max_read_len, int n_qual, int avg_reads, int n_haps, int32_t out[10])
{
    int rc = check_params(p);
    if (rc) return rc;
    if (!out) return fail(DD_ERR_INVALID, "null argument");
    if (max_hap_len < 1 || max_hap_len > DD_MAX_HAP_LEN) return fail(DD_ERR_UNSUPPORTED, "haplotype length outside [1,766]");
    if (max_read_len < 1 || max_read_len > DD_MAX_READ_LEN) return fail(DD_ERR_UNSUPPORTED, "read length outside [1,1024]");
    // the shape of a whole-batch launch over n_haps haplotypes in windows of avg_reads reads, with all the workspace it may want
    LaunchAsk ask;
    ask.p = p; ask.n_windows = 1; ask.n_haps = n_haps; ask.n_reads = avg_reads; ask.max_hap_len = max_hap_len; ask.max_read_len = max_read_len;
    ask.n_qual = n_qual; ask.workspace_bytes = ~(size_t)0;
    LaunchShape s;
    ddk::KernelArgs A;
    memset(&A, 0, sizeof(A));
    if ((rc = shape_launch(read_switches(), ask, s, A))) return rc;
    const int32_t v[10] = {s.pl.K, s.pl.Dt, s.pl.gbt ? 1 : 0, s.waves, (int32_t)s.split, (int32_t)s.lds, (int32_t)((s.pl.scratch_bytes >> 10) & 0x7fffffff),
                           s.pl.waves_per_cu, s.pl.G, 0};
    memcpy(out, v, sizeof(v));
    return DD_SUCCESS;
}
} // extern "C"
