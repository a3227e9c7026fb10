// align_events_kernel.hip — the indel events of an alignment, from what dd_hapalign_kernel leaves in HBM: per pair its status and its
// int16 slice of reference offsets (dd_align_result).  Per pair it writes the events convertAlignment (reference
// ObservationModelSeqAn.hpp:142-269) would put into hap.indels — keys, types, lengths and read positions (dd_align_events) — so that a
// caller who only asks "which indels, and where" copies back a few records instead of the slice and walks nothing on the host.
//
// Per haplotype base b: upto = reference bases left of its column (p if paired, DD_ALIGN_GAP_REFS(p) if it faces a gap), nxt = reference
// bases consumed by the bases before it (p' + 1 behind a paired base, upto' behind a gap-facing one, 0 at the start).
//     deletion   upto > nxt and a paired base was seen before b (fbfound): {DEL, nxt, upto - nxt, b}
//     insertion  b starts a maximal run of gap-facing bases with one upto = n, 0 < n < reference length: {INS, n, run, b}
//                (n == 0 is the leading run, LO; n == reference length is RO: neither is recorded)
// Both tests need only the base's own value and its predecessor's, so 64 bases are classified at a time: a lane gets its predecessor by a
// wave shift (lane 0: the previous chunk's lane 63, carried as a scalar), event starts are ballots, slots a prefix popcount (a deletion
// in front of base b before an insertion starting at b), the run length the count of continuation bits behind the start.  A run that
// reaches the end of its chunk keeps its slot and is written once a later chunk ends it.  fbfound is carried as a scalar.
//
// Mapping: one wavefront per pair, DD_ALIGN_WAVES per workgroup, a persistent grid that draws pairs from a counter in the alignment
// workspace's header, drawn the way dd_hapalign_kernel draws (every lane takes part; see there).
//
// Memory safety: only status[pair], the offsets of the pair and ref_pos[hap_off[pair] ... hap_off[pair + 1]) are read, the values read
// index nothing; stores go to n_events[pair] and to events[pair * events_cap + slot] with slot < events_cap.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "align_events_kernel.h"

namespace dda {
namespace {

__device__ __forceinline__ unsigned long long event_word(int kind, int ref, int len, int hap)
{
    return (unsigned long long)(uint16_t)kind | ((unsigned long long)(uint16_t)ref << 16) | ((unsigned long long)(uint16_t)len << 32) |
           ((unsigned long long)(uint16_t)hap << 48);        // dd_align_events {kind, ref, len, hap}, little endian
}

} // namespace

__global__ void __launch_bounds__(64 * DD_ALIGN_WAVES) dd_align_events_kernel(EventsArgs P)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long lanes_below = (1ull << lane) - 1ull;
    unsigned int *counter = P.hdr + DD_EVENTS_HDR_COUNTER;

    unsigned int draws = 0;                                     // pairs this wavefront drew: at most n_pairs if the draw stays wave-uniform
    for (;;) {
        unsigned int drawn = atomicAdd(counter, lane == 0 ? 1u : 0u);          // every lane takes part in the draw (hapalign_kernel.hip)
        drawn = __builtin_amdgcn_readfirstlane(drawn);
        if (drawn >= (unsigned int)P.n_pairs) break;
        if (++draws > (unsigned int)P.n_pairs) {                // run-time guard of the draw (dd_align_events_last_launch reports it)
            if (lane == 0) atomicAdd(P.hdr + DD_EVENTS_HDR_TRIPS, 1u);
            break;
        }
        const int pair = (int)drawn;
        const int r = P.pair_ref[pair];
        const bool ok = P.status[pair] == DD_ALIGN_OK && r >= 0 && r < P.n_refs;
        const int h0 = P.hap_off[pair];
        const int len2 = ok ? P.hap_off[pair + 1] - h0 : 0;     // a pair that was not aligned has no events: its loop does not run
        const int hlen = ok ? P.ref_off[r + 1] - P.ref_off[r] : 0;
        const int16_t *rp = P.ref_pos + h0;
        unsigned long long *ev = reinterpret_cast<unsigned long long *>(P.events) + (size_t)pair * (size_t)P.events_cap;

        int n_ev = 0;                                           // events so far (wave-uniform, like everything carried between chunks)
        int c_upto = 0, c_gap = 1;                              // the base in front of the chunk: "a gap-facing base with upto 0" makes nxt 0 at the start
        bool fb = false;                                        // a paired base lies in an earlier chunk
        bool pend = false;                                      // an insertion that reached the end of its chunk, not yet written
        int pend_slot = 0, pend_ref = 0, pend_len = 0, pend_hap = 0;
        for (int base = 0; base < len2; base += 64) {
            const int b = base + lane;
            const bool valid = b < len2;
            const int p = valid ? (int)rp[b] : 0;
            const bool gap = valid && p < 0;
            const int upto = p < 0 ? -1 - p : p;
            int pv_upto = __shfl_up(upto, 1), pv_gap = __shfl_up((int)gap, 1);
            if (lane == 0) { pv_upto = c_upto; pv_gap = c_gap; }
            const int nxt = pv_gap ? pv_upto : pv_upto + 1;
            const unsigned long long paired_mask = __ballot(valid && p >= 0);
            const bool del = valid && upto > nxt && (fb || (paired_mask & lanes_below) != 0);
            const bool ins_base = gap && upto > 0 && upto < hlen;                // a base of a recorded insertion
            const bool cont = ins_base && pv_gap && pv_upto == upto;              // ... that continues its predecessor's run
            const bool start = ins_base && !cont;
            const unsigned long long cont_mask = __ballot(cont), del_mask = __ballot(del), start_mask = __ballot(start);

            if (pend) {                                         // the chunk's leading continuation bits belong to the pending run
                const int c = ~cont_mask == 0 ? 64 : __builtin_ctzll(~cont_mask);
                pend_len += c;
                if (c < 64) {
                    if (lane == 0 && pend_slot < P.events_cap) ev[pend_slot] = event_word(DD_ALIGN_EVENT_INS, pend_ref, pend_len, pend_hap);
                    pend = false;
                }
            }
            const int run = 1 + __builtin_ctzll(~(lane == 63 ? 0ull : cont_mask >> (lane + 1)));
            const bool open_end = start && lane + run == 64;    // at most one lane: the run goes on into the next chunk, or ends with this one
            const int slot_del = n_ev + __popcll(del_mask & lanes_below) + __popcll(start_mask & lanes_below);
            const int slot_ins = slot_del + (del ? 1 : 0);
            if (del && slot_del < P.events_cap) ev[slot_del] = event_word(DD_ALIGN_EVENT_DEL, nxt, upto - nxt, b);
            if (start && !open_end && slot_ins < P.events_cap) ev[slot_ins] = event_word(DD_ALIGN_EVENT_INS, upto, run, b);
            const unsigned long long open_mask = __ballot(open_end);
            if (open_mask) {
                const int src = __builtin_ctzll(open_mask);
                pend = true;
                pend_slot = __builtin_amdgcn_readfirstlane(__shfl(slot_ins, src));
                pend_ref = __builtin_amdgcn_readfirstlane(__shfl(upto, src));
                pend_len = __builtin_amdgcn_readfirstlane(__shfl(run, src));
                pend_hap = base + src;
            }
            n_ev += __popcll(del_mask) + __popcll(start_mask);
            fb = fb || paired_mask != 0;
            c_upto = __builtin_amdgcn_readlane(upto, 63);
            c_gap = __builtin_amdgcn_readlane((int)gap, 63);
        }
        if (pend && lane == 0 && pend_slot < P.events_cap) ev[pend_slot] = event_word(DD_ALIGN_EVENT_INS, pend_ref, pend_len, pend_hap);
        if (lane == 0) P.n_events[pair] = n_ev;
    }
    if (lane == 0) atomicMax(P.hdr + DD_EVENTS_HDR_MAX_DRAWS, draws);
}

hipError_t launch_align_events(const EventsArgs &A, hipStream_t st)
{
    if (A.n_pairs <= 0) return hipSuccess;
    return zero_and_launch(dd_align_events_kernel, persistent_grid(A.n_pairs, DD_ALIGN_WAVES, DD_ALIGN_MAX_BLOCKS), 64 * DD_ALIGN_WAVES, 0,
                           A.hdr + DD_EVENTS_HDR_BASE, DD_DRAW_WORDS * sizeof(unsigned int), st, A);
}

} // namespace dda
