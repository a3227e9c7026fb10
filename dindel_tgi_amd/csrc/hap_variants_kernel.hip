// hap_variants_kernel.hip — the variants of an alignment, from what dd_hapalign_kernel leaves in HBM (per pair its status and its int16
// slice of reference offsets) and the two sequences: per pair a summary and, in column order, one fixed-size record per variant
// (dd_hap_variants_summary, dd_hap_variant) — everything convertAlignment (reference ObservationModelSeqAn.hpp:142-269) and
// Realign::getFlankingCoordinatesBetter (:37-139) give for a haplotype except the strings, which the host forms from the sequences by
// position.  host/align_haplotypes.cpp: hapVariantsHost is this kernel's twin on the host, word for word.
//
// Classification (the rules of align_events_kernel.hip, extended).  Per haplotype base b: upto = reference bases left of its column (p if
// paired, DD_ALIGN_GAP_REFS(p) if it faces a gap), nxt = reference bases consumed by the bases before it.
//     deletion    upto > nxt: {DEL, nxt, upto - nxt, startRead b - 1} once a paired base was seen before b (fbfound); before that
//                 {DEL_UNSEEN, ...}: convertAlignment marks the bases 'D' in hap.align and records nothing
//     insertion   b starts a maximal run of gap-facing bases with one upto = n, 0 < n < S (the reference length): {INS, n, run, b}
//                 (n == 0 is the leading run, LO; n == S is RO: neither is recorded)
//     SNP         b is paired with reference base p and the two seqan::Dna letters differ: {SNP, p, 1, b}
// A deletion in front of base b comes before what b itself gives.  Reference bases behind the last haplotype base give nothing.
// firstBase = p of the first paired base (-1: none), lastBase = nxt behind the last base.
//
// Flanks in closed form.  getFlankingCoordinatesBetter compares whole strings: for a deletion of l bases at sh it erases l bases at
// every x and asks whether the result equals the result of erasing at sh.  With E_x = ref[0, x) + ref[x + l, S):
//   x < sh: E_x and E_sh agree outside [x, sh); inside, E_x[i] = ref[i + l] and E_sh[i] = ref[i].  Equal iff ref[i] == ref[i + l] for all
//           i in [x, sh).  So the qualifying x are contiguous below sh: with runL = the number of consecutive i = sh - 1, sh - 2, ... >= 1
//           (the loop stops at x > 0) with ref[i] == ref[i + l], the last assignment is leftFlankHap = sh - runL - 1 (also for runL = 0).
//   x > sh: inside [sh, x) E_sh[i] = ref[i + l], E_x[i] = ref[i]: the same test over [sh, x).  The loop runs for x < S - l, so with runR
//           consecutive i = sh, sh + 1, ... the last qualifying x is max(sh, min(sh + runR, S - l - 1)) and rightFlankHap = x + l.
// For an insertion of l bases at sh let O = ref[0, sh) + ins + ref[sh, S) (the inserted letters as seqan::Dna letters, the reference raw,
// as the reference code mixes them); it inserts O[x, x + l) at x into ref and compares with O:
//   x < sh: the result agrees with O on [0, x + l) by construction and on [sh + l, S + l) because both hold ref[i - l] there; on
//           [x + l, sh + l) it holds ref[i - l].  Equal iff ref[j] == O[j + l] for all j in [x, sh): leftFlankHap = sh - runL - 1 again.
//   x > sh: it agrees on [x, S + l) and on [0, sh); on [sh, x) it holds ref[i].  Equal iff ref[i] == O[i] for all i in [sh, x):
//           rightFlankHap = max(sh, min(sh + runR, S - l - 1)).
// Both loops bound x by `x < int(hapSeq.size() - l)` in unsigned arithmetic: for l > S that wraps, and nothing here restates it — an
// insertion with l >= S sets DD_HAP_VARIANTS_HOST, its flanks stay 0 and the host converts the pair from its slice.  (A deletion has
// l <= S: its bases are the reference's.)  The read flanks and the clamps follow as in the reference, quirks included: leftFlankHap <= 0
// becomes 0; leftFlankRead < 0 becomes 0; rightFlankRead >= readSize assigns leftFlankRead (leftFlankHap in the SNP's haplotype test).
// A run is counted 64 comparisons at a time: a ballot of the equal positions, its trailing ones.
//
// Mapping: one wavefront per pair, DD_ALIGN_WAVES per workgroup, a persistent grid that draws pairs from a counter in the alignment
// workspace's header (words of its own), drawn the way dd_hapalign_kernel draws.  64 bases are classified per step as in
// align_events_kernel.hip (predecessor by wave shift, carries as scalars, slots from prefix popcounts, an insertion that reaches the end of
// its chunk pending).  SNP and DEL_UNSEEN records are written by their lanes; deletions and insertions one after the other by the whole
// wavefront, on scalar state, because their flank searches are wave-wide.
//
// Memory safety: every load is guarded by the pair's own lengths, not by the slice's values (p < S for a SNP, i + l < S in the flank
// searches, an insertion's letters lie inside its own run); stores go to summary[pair] and variants[pair * cap + slot], 0 <= slot < cap.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hap_variants_kernel.h"

namespace dda {
namespace {

typedef unsigned long long u64;

__device__ __forceinline__ u64 pack4(int a, int b, int c, int d)
{
    return (u64)(uint16_t)a | ((u64)(uint16_t)b << 16) | ((u64)(uint16_t)c << 32) | ((u64)(uint16_t)d << 48);     // four int16, little endian
}

__device__ __forceinline__ int dna_letter(uint8_t c)             // seqan::Dna as a letter (host dnaLetter)
{
    const int l = c | 0x20;
    return l == 'c' ? 'C' : l == 'g' ? 'G' : (l == 't' || l == 'u') ? 'T' : 'A';
}

// the number of leading k = 0, 1, 2, ... with eq(k), counted by the whole wavefront (eq must be false beyond a finite range)
template <class Eq> __device__ __forceinline__ int count_run(int lane, Eq eq)
{
    int run = 0;
    for (int base = 0;; base += 64) {
        const u64 m = __ballot(eq(base + lane));
        const int c = ~m == 0 ? 64 : __builtin_ctzll(~m);
        run += c;
        if (c < 64) break;
    }
    return run;
}

// the two words of a record from its flanks in the haplotype (getFlankingCoordinatesBetter's last lines)
__device__ __forceinline__ u64 flank_word(int start_read, int sh, int rlen, int lfh, int rfh, int right_of_read)
{
    if (lfh <= 0) lfh = 0;
    int lfr = start_read - (sh - lfh) + 1;
    if (lfr < 0) lfr = 0;
    const int rfr = right_of_read + (rfh - sh);
    if (rfr >= rlen) lfr = rlen - 1;
    return pack4(lfh, rfh, lfr, rfr);
}

struct PairView { const uint8_t *ref, *hap; int S, rlen; u64 *rec; int cap; };

// wave-uniform arguments; every lane computes the same words, lane 0 stores them
__device__ __forceinline__ void deletion_record(const PairView &V, int lane, int slot, int sh, int l, int b)
{
    const uint8_t *ref = V.ref;
    const int S = V.S;
    const int runL = count_run(lane, [&](int k) { const int j = sh - 1 - k; return j >= 1 && j + l < S && ref[j] == ref[j + l]; });
    const int runR = count_run(lane, [&](int k) { const int i = sh + k; return i + l < S && ref[i] == ref[i + l]; });
    const int xmax = max(sh, min(sh + runR, S - l - 1));
    if (lane == 0 && slot < V.cap) {
        V.rec[2 * slot] = pack4(DD_ALIGN_EVENT_DEL, sh, l, b - 1);
        V.rec[2 * slot + 1] = flank_word(b - 1, sh, V.rlen, sh - runL - 1, xmax + l, b - l);
    }
}

// returns DD_HAP_VARIANTS_HOST when the flanks have no closed form
__device__ __forceinline__ int insertion_record(const PairView &V, int lane, int slot, int sh, int l, int b)
{
    const uint8_t *ref = V.ref, *ins = V.hap + b;                // ins[0 ... l): the run's own bases
    const int S = V.S;
    u64 flanks = 0;
    const bool host = l >= S;
    if (!host) {
        const int runL = count_run(lane, [&](int k) {
            const int j = sh - 1 - k, kk = j + l;                // O[kk], kk < sh + l
            return j >= 1 && (int)ref[j] == (kk < sh ? (int)ref[kk] : dna_letter(ins[kk - sh]));
        });
        const int runR = count_run(lane, [&](int k) {
            const int i = sh + k;                                // O[i], i >= sh
            return i < S && (int)ref[i] == (i < sh + l ? dna_letter(ins[i - sh]) : (int)ref[i - l]);
        });
        const int xmax = max(sh, min(sh + runR, S - l - 1));
        flanks = flank_word(b, sh, V.rlen, sh - runL - 1, xmax, b + l);
    }
    if (lane == 0 && slot < V.cap) {
        V.rec[2 * slot] = pack4(DD_ALIGN_EVENT_INS, sh, l, b);
        V.rec[2 * slot + 1] = flanks;
    }
    return host ? DD_HAP_VARIANTS_HOST : 0;
}

} // namespace

__global__ void __launch_bounds__(64 * DD_ALIGN_WAVES) dd_hap_variants_kernel(VariantsArgs P)
{
    const int lane = threadIdx.x & 63;
    const u64 lanes_below = (1ull << lane) - 1ull;
    unsigned int *counter = P.hdr + DD_VARIANTS_HDR_COUNTER;

    unsigned int draws = 0;                                     // pairs this wavefront drew: at most n_pairs if the draw stays wave-uniform
    for (;;) {
        unsigned int drawn = atomicAdd(counter, lane == 0 ? 1u : 0u);          // every lane takes part in the draw (hapalign_kernel.hip)
        drawn = __builtin_amdgcn_readfirstlane(drawn);
        if (drawn >= (unsigned int)P.n_pairs) break;
        if (++draws > (unsigned int)P.n_pairs) {                // run-time guard of the draw (dd_hap_variants_last_launch reports it)
            if (lane == 0) atomicAdd(P.hdr + DD_VARIANTS_HDR_TRIPS, 1u);
            break;
        }
        const int pair = (int)drawn;
        const int r = P.pair_ref[pair];
        const bool ok = P.status[pair] == DD_ALIGN_OK && r >= 0 && r < P.n_refs;
        const int h0 = P.hap_off[pair];
        const int len2 = ok ? P.hap_off[pair + 1] - h0 : 0;     // a pair that was not aligned has no records: its loop does not run
        const int r0 = ok ? P.ref_off[r] : 0;
        const int S = ok ? P.ref_off[r + 1] - r0 : 0;
        const int16_t *rp = P.ref_pos + h0;
        PairView V;
        V.ref = P.ref_seq + r0; V.hap = P.hap_seq + h0; V.S = S; V.rlen = len2; V.cap = P.cap;
        V.rec = reinterpret_cast<u64 *>(P.variants) + 2 * (size_t)pair * (size_t)P.cap;

        int n_ev = 0;                                           // records so far (wave-uniform, like everything carried between chunks)
        int c_upto = 0, c_gap = 1;                              // the base in front of the chunk: "a gap-facing base with upto 0" makes nxt 0 at the start
        bool fb = false;                                        // a paired base lies in an earlier chunk
        int first_base = -1, last_base = 0, flags = 0;
        bool pend = false;                                      // an insertion that reached the end of its chunk, not yet written
        int pend_slot = 0, pend_ref = 0, pend_len = 0, pend_hap = 0;
        for (int base = 0; base < len2; base += 64) {
            const int b = base + lane;
            const bool valid = b < len2;
            const int p = valid ? (int)rp[b] : 0;
            const bool gap = valid && p < 0;
            const bool paired = valid && p >= 0;
            const int upto = p < 0 ? -1 - p : p;
            int pv_upto = __shfl_up(upto, 1), pv_gap = __shfl_up((int)gap, 1);
            if (lane == 0) { pv_upto = c_upto; pv_gap = c_gap; }
            const int nxt = pv_gap ? pv_upto : pv_upto + 1;
            const u64 paired_mask = __ballot(paired);
            const bool seen = fb || (paired_mask & lanes_below) != 0;             // fbfound in front of base b
            const bool del = valid && upto > nxt;
            const bool ins_base = gap && upto > 0 && upto < S;                    // a base of a recorded insertion
            const bool cont = ins_base && pv_gap && pv_upto == upto;              // ... that continues its predecessor's run
            const bool start = ins_base && !cont;
            const bool inRef = paired && p < S;                                   // (an aligned pair's offsets always are)
            const bool snp = inRef && dna_letter(V.hap[b]) != dna_letter(V.ref[p]);
            const u64 cont_mask = __ballot(cont), del_mask = __ballot(del), start_mask = __ballot(start), snp_mask = __ballot(snp);
            const u64 own_mask = start_mask | snp_mask;

            if (pend) {                                         // the chunk's leading continuation bits belong to the pending run
                const int c = ~cont_mask == 0 ? 64 : __builtin_ctzll(~cont_mask);
                pend_len += c;
                if (c < 64) {
                    flags |= insertion_record(V, lane, pend_slot, pend_ref, pend_len, pend_hap);
                    pend = false;
                }
            }
            const int run = 1 + __builtin_ctzll(~(lane == 63 ? 0ull : cont_mask >> (lane + 1)));
            const bool open_end = start && lane + run == 64;    // at most one lane: the run goes on into the next chunk, or ends with this one
            const int slot_del = n_ev + __popcll(del_mask & lanes_below) + __popcll(own_mask & lanes_below);
            const int slot_own = slot_del + (del ? 1 : 0);
            if (del && !seen && slot_del < V.cap) {             // marked 'D' in hap.align, not a variant: no flanks
                V.rec[2 * slot_del] = pack4(DD_HAP_VARIANT_DEL_UNSEEN, nxt, upto - nxt, b - 1);
                V.rec[2 * slot_del + 1] = 0;
            }
            if (snp && slot_own < V.cap) {                      // getFlankingCoordinatesBetter's last branch
                int lfr = b - 1; if (lfr < 0) lfr = 0;
                const int rfr = b + 1; if (rfr >= len2) lfr = len2 - 1;
                int lfh = p - 1; if (lfh < 0) lfh = 0;
                const int rfh = p + 1; if (rfh >= S) lfh = S - 1;
                V.rec[2 * slot_own] = pack4(DD_HAP_VARIANT_SNP, p, 1, b);
                V.rec[2 * slot_own + 1] = pack4(lfh, rfh, lfr, rfr);
            }
            const u64 open_mask = __ballot(open_end);
            // the recorded deletions and the insertions that end in this chunk, one after the other on scalar state
            for (u64 m = __ballot(del && seen); m; m &= m - 1) {
                const int src = __builtin_ctzll(m);
                const int slot = __builtin_amdgcn_readfirstlane(__shfl(slot_del, src));
                const int sh = __builtin_amdgcn_readfirstlane(__shfl(nxt, src));
                const int to = __builtin_amdgcn_readfirstlane(__shfl(upto, src));
                deletion_record(V, lane, slot, sh, to - sh, base + src);
            }
            for (u64 m = start_mask & ~open_mask; m; m &= m - 1) {
                const int src = __builtin_ctzll(m);
                const int slot = __builtin_amdgcn_readfirstlane(__shfl(slot_own, src));
                const int sh = __builtin_amdgcn_readfirstlane(__shfl(upto, src));
                const int l = __builtin_amdgcn_readfirstlane(__shfl(run, src));
                flags |= insertion_record(V, lane, slot, sh, l, base + src);
            }
            if (open_mask) {
                const int src = __builtin_ctzll(open_mask);
                pend = true;
                pend_slot = __builtin_amdgcn_readfirstlane(__shfl(slot_own, src));
                pend_ref = __builtin_amdgcn_readfirstlane(__shfl(upto, src));
                pend_len = __builtin_amdgcn_readfirstlane(__shfl(run, src));
                pend_hap = base + src;
            }
            n_ev += __popcll(del_mask) + __popcll(own_mask);
            if (!fb && paired_mask) first_base = __builtin_amdgcn_readfirstlane(__shfl(p, __builtin_ctzll(paired_mask)));
            fb = fb || paired_mask != 0;
            if (base == 0 && __builtin_amdgcn_readfirstlane(p) == -1) flags |= DD_HAP_VARIANTS_LO_FIRST;       // (lane 0 is valid: len2 >= 1)
            if (base + 64 >= len2) {                            // the chunk of the last base
                const int src = len2 - 1 - base;
                const int lp = __builtin_amdgcn_readfirstlane(__shfl(p, src));
                last_base = lp < 0 ? -1 - lp : lp + 1;
                if (len2 > 1 && lp < 0 && -1 - lp == S) flags |= DD_HAP_VARIANTS_RO_LAST;
            }
            c_upto = __builtin_amdgcn_readlane(upto, 63);
            c_gap = __builtin_amdgcn_readlane((int)gap, 63);
        }
        if (pend) flags |= insertion_record(V, lane, pend_slot, pend_ref, pend_len, pend_hap);
        if (lane == 0) {
            dd_hap_variants_summary s;
            s.n_variants = n_ev; s.first_base = ok ? first_base : 0; s.last_base = last_base; s.flags = flags;
            P.summary[pair] = s;
        }
    }
    if (lane == 0) atomicMax(P.hdr + DD_VARIANTS_HDR_MAX_DRAWS, draws);
}

hipError_t launch_hap_variants(const VariantsArgs &A, hipStream_t st)
{
    if (A.n_pairs <= 0) return hipSuccess;
    return zero_and_launch(dd_hap_variants_kernel, persistent_grid(A.n_pairs, DD_ALIGN_WAVES, DD_ALIGN_MAX_BLOCKS), 64 * DD_ALIGN_WAVES, 0,
                           A.hdr + DD_VARIANTS_HDR_BASE, DD_DRAW_WORDS * sizeof(unsigned int), st, A);
}

} // namespace dda
