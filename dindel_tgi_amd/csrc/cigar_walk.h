// cigar_walk.h — the CIGAR walk of one (haplotype, read) pair by one wavefront: the body that cigar_kernel.hip (every pair, written at the
// pair's index) and realign_kernel.hip (the pair chosen for a read, written at the read's index) share.  The walk exists here and nowhere
// else; cigar_kernel.hip's head comment describes it.
#ifndef DD_CIGAR_WALK_H
#define DD_CIGAR_WALK_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cigar_kernel.h"

namespace ddc {
namespace {

enum { CLS_NONE = 0, CLS_GOES_ON, CLS_CONSEC, CLS_REF_TO_INS, CLS_IMPOSSIBLE, CLS_DEL, CLS_INS_TO_REF, CLS_INS_DEL };   // events: >= CLS_REF_TO_INS

// position on the reference of read base b (host/cigar.cpp:14).  An inserted base carries its key in hpos (DD_HPOS_INS_KEY0 - pos): that is
// MLAlignment::INS here.  The host indexes hapRefPos without a check; an index beyond the haplotype reads its last base instead of memory
// that is not the haplotype's.  Bases beyond the read get a code without a position: nothing looks at them (b <= last < L).
__device__ __forceinline__ int on_ref(const int16_t *hp, const int32_t *href, int Hs, int b, int L)
{
    if (b >= L || Hs <= 0) return DD_HPOS_LO;
    const int v = hp[b];
    if (v >= 0) return href[v < Hs ? v : Hs - 1];
    return v < DD_HPOS_INS_KEY0 ? DD_HPOS_INS : v;
}

__device__ __forceinline__ uint64_t bits_below(int n) { return n >= 64 ? ~0ull : ((1ull << n) - 1ull); }

// the pair's operation list (wave-uniform state; lane 0 stores): every operation counts, the first `cap` are written
struct OpList {
    uint32_t *ops;
    int cap, n, lane;
    __device__ __forceinline__ void push(int op, int len)
    {
        if (n < cap && lane == 0) ops[n] = ((uint32_t)len << 4) | (uint32_t)op;
        n++;
    }
};

// The CIGAR of `pair` (wave-uniform), written to out.status / n_ops / ref_off [at] and out.ops [at * ops_cap].  Every lane of the wavefront
// calls it with the same arguments.
__device__ __forceinline__ void cigar_walk(const CigarArgs &P, const int64_t pair, const dd_cigar_result &out, const int64_t at, const int lane)
{
    if (P.pair_status && P.pair_status[pair] != DD_PAIR_OK) {     // no alignment was computed: marked, hpos not read, ops not written
        if (lane == 0) { out.status[at] = DD_CIGAR_NOT_COMPUTED; out.n_ops[at] = 0; out.ref_off[at] = -1; }
        return;
    }
    int lo = 0, hi = P.n_windows;                                  // window of this pair: binary search in the pair offsets
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (P.win_pair_off[mid] <= pair) lo = mid; else hi = mid;
    }
    const int w = lo;
    const int q0 = P.win_read_off[w], R = P.win_read_off[w + 1] - q0;
    const int idx = (int)(pair - P.win_pair_off[w]);
    const int h = idx / R, r = idx - h * R;
    const int g = P.win_hap_off[w] + h, q = q0 + r;
    const int rs0 = P.read_seq_off[q0], SL = P.read_seq_off[q0 + R] - rs0;
    const int rb = P.read_seq_off[q], L = P.read_seq_off[q + 1] - rb;
    const int16_t *hp = P.hpos + P.win_hpos_off[w] + (int64_t)h * SL + (rb - rs0);
    const int hb = P.hap_seq_off[g], Hs = P.hap_seq_off[g + 1] - hb;
    const int32_t *href = P.hap_ref_pos + hb;
    OpList ops = {out.ops + at * (int64_t)P.ops_cap, P.ops_cap, 0, lane};
    int status = DD_CIGAR_OK, ref_off = -1;

    if (P.hap_aligned && !P.hap_aligned[g]) {
        status = DD_CIGAR_HAP_NOT_ALIGNED;
    } else {
        // last base with a position: chunks from the end (the last chunk nearly always has one); its values stay in `cur`
        int last = -1, cur_c0 = -64, cur = DD_HPOS_LO;
        for (int c0 = L > 0 ? ((L - 1) & ~63) : -64; c0 >= 0; c0 -= 64) {
            cur = on_ref(hp, href, Hs, c0 + lane, L); cur_c0 = c0;
            const uint64_t m = __ballot(cur >= 0);
            if (m) { last = c0 + 63 - __builtin_clzll(m); break; }
        }
        if (last < 0) {
            ops.push(CIG_SOFT_CLIP, L);                            // nothing aligned: the whole read is clipped, no position
        } else {
            int first = -1, op = CIG_MATCH, len = 1;
            int carry = DD_HPOS_LO;                                // onRef of the base in front of this chunk
            int carry_anchor = 0;                                  // onRef of the nearest base in front of this chunk that is not INS
            for (int c0 = 0; c0 <= last && status == DD_CIGAR_OK; c0 += 64) {
                if (c0 != cur_c0) { cur = on_ref(hp, href, Hs, c0 + lane, L); cur_c0 = c0; }
                const int b = c0 + lane;
                if (first < 0) {                                   // leading bases without a position are clipped
                    const uint64_t m = __ballot(cur >= 0);
                    if (m) {
                        const int f = __builtin_ctzll(m);
                        first = c0 + f;
                        ref_off = __builtin_amdgcn_readlane(cur, f);
                        if (first > 0) ops.push(CIG_SOFT_CLIP, first);
                    }
                }
                int prev = __shfl_up(cur, 1);
                if (lane == 0) prev = carry;
                const uint64_t notins = __ballot(cur != DD_HPOS_INS);
                const uint64_t before = notins & bits_below(lane);
                int anchor = __shfl(cur, before ? 63 - __builtin_clzll(before) : 0);
                if (!before) anchor = carry_anchor;
                int cls = CLS_NONE, gap = 0;
                if (first >= 0 && b > first && b <= last) {        // the step (b-1) -> b
                    if (cur == DD_HPOS_INS) {
                        cls = prev == DD_HPOS_INS ? CLS_GOES_ON : prev >= 0 ? CLS_REF_TO_INS : CLS_IMPOSSIBLE;
                    } else if (prev >= 0 && cur >= 0) {
                        const int d = cur - prev;
                        cls = d == 1 ? CLS_CONSEC : d > 1 ? CLS_DEL : CLS_NONE;
                        gap = d - 1;
                    } else if (prev == DD_HPOS_INS) {
                        const int d = (int)((uint32_t)cur - (uint32_t)anchor);
                        cls = d == 1 ? CLS_INS_TO_REF : d > 1 ? CLS_INS_DEL : CLS_NONE;
                        gap = d - 1;
                    }
                }
                const uint64_t m_on = __ballot(cls == CLS_GOES_ON), m_consec = __ballot(cls == CLS_CONSEC);
                uint64_t ev = __ballot(cls >= CLS_REF_TO_INS);
                int from = 0;
                for (;;) {
                    const int e = ev ? __builtin_ctzll(ev) : 64;
                    const uint64_t stretch = bits_below(e) & ~bits_below(from);
                    const int n_on = __builtin_popcountll(m_on & stretch), n_consec = __builtin_popcountll(m_consec & stretch);
                    if (op == CIG_MATCH) {
                        if (n_on) { status = DD_CIGAR_ERROR1; break; }
                        len += n_consec;
                    } else {
                        if (n_consec) { status = DD_CIGAR_ERROR3; break; }
                        len += n_on;
                    }
                    if (e == 64) break;
                    const int c = __builtin_amdgcn_readlane(cls, e), gp = __builtin_amdgcn_readlane(gap, e);
                    if (c == CLS_REF_TO_INS) {
                        if (op != CIG_MATCH) { status = DD_CIGAR_ERROR2; break; }
                        ops.push(CIG_MATCH, len);
                        op = CIG_INS; len = 1;
                    } else if (c == CLS_IMPOSSIBLE) {
                        status = DD_CIGAR_IMPOSSIBLE; break;
                    } else if (c == CLS_DEL) {
                        if (op != CIG_MATCH) { status = DD_CIGAR_ERROR4; break; }
                        ops.push(CIG_MATCH, len);
                        ops.push(CIG_DEL, gp);
                        len = 1;
                    } else {                                       // INS -> reference, with or without skipped reference bases
                        ops.push(CIG_INS, len);
                        if (c == CLS_INS_DEL) ops.push(CIG_DEL, gp);
                        op = CIG_MATCH; len = 1;
                    }
                    ev &= ev - 1;
                    from = e + 1;
                }
                carry = __builtin_amdgcn_readlane(cur, 63);
                if (notins) carry_anchor = __builtin_amdgcn_readlane(cur, 63 - __builtin_clzll(notins));
            }
            if (status == DD_CIGAR_OK) {
                ops.push(op, len);
                if (L - 1 - last > 0) ops.push(CIG_SOFT_CLIP, L - 1 - last);
            }
        }
    }
    if (status == DD_CIGAR_OK && ops.n > P.ops_cap) status = DD_CIGAR_OVERFLOW;
    if (lane == 0) {
        const bool thrown = status != DD_CIGAR_OK && status != DD_CIGAR_OVERFLOW;
        out.status[at] = status;
        out.n_ops[at] = thrown ? 0 : ops.n;
        out.ref_off[at] = thrown ? -1 : ref_off;
    }
}

} // namespace
} // namespace ddc
#endif
