// arena_layout_check — the layout of the one-shot arena on its own: capi_internal.h's arena_layout / arena_point over lists of slots, linked
// with nothing of the library (no kernel unit, no device).  The expected numbers follow from the rule (every piece starts at a multiple of
// 256 bytes, an array of 0 bytes takes 1) and are written out here.  Prints one line per difference and "arena_layout_check: N checks ok"
// when there is none.
#include "../dindel_tgi_amd/csrc/capi_internal.h"

using namespace ddh;

static int g_checks = 0, g_failed = 0;

static void expect(const char *what, size_t i, unsigned long long got, unsigned long long want)
{
    g_checks++;
    if (got == want) return;
    std::printf("%s[%zu] is %llu, expected %llu\n", what, i, got, want);
    g_failed++;
}

static void expect_layout(const char *what, const std::vector<ArenaSlot> &slots, const std::vector<size_t> &want_off, size_t want_total)
{
    std::vector<size_t> off(3, 12345);       // whatever it held is replaced
    const size_t total = arena_layout(slots, off);
    expect(what, 999, total, want_total);
    expect(what, 998, off.size(), want_off.size());
    for (size_t i = 0; i < off.size() && i < want_off.size(); i++) expect(what, i, off[i], want_off[i]);
}

int main()
{
    // sizes {0, 1, 256, 257}, each variable of a pointer type of its own
    const int32_t *a = nullptr; char *b = nullptr; const double *c = nullptr; dd_align_events *d = nullptr;
    const std::vector<ArenaSlot> four = {arena_slot(&a, 0), arena_slot(&b, 1), arena_slot(&c, 256), arena_slot(&d, 257)};
    expect_layout("four", four, {0, 256, 512, 768}, 1280);
    expect_layout("empty", {}, {}, 0);

    // every variable ends up at base + its offset, written through its own type
    std::vector<size_t> off;
    std::vector<unsigned char> mem(arena_layout(four, off));
    arena_point(four, off, mem.data());
    expect("var", 0, reinterpret_cast<uintptr_t>(a), reinterpret_cast<uintptr_t>(mem.data()));
    expect("var", 1, reinterpret_cast<uintptr_t>(b), reinterpret_cast<uintptr_t>(mem.data() + 256));
    expect("var", 2, reinterpret_cast<uintptr_t>(c), reinterpret_cast<uintptr_t>(mem.data() + 512));
    expect("var", 3, reinterpret_cast<uintptr_t>(d), reinterpret_cast<uintptr_t>(mem.data() + 768));
    b[0] = 1; d[0].kind = 2;           // and is the caller's to use (the sanitizers watch)

    // the 13 arrays of the alignment's host entry for P = 3 pairs, R = 2 references, 10 reference bytes, 17 haplotype bytes and a workspace
    // of 4,352 bytes, without events or variants: the sequence of `take` calls the entry used to make, by hand
    const size_t P = 3, R = 2, ref_bytes = 10, hap_bytes = 17, ws_bytes = 4352;
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t o = at; at = (at + (bytes > 1 ? bytes : 1) + 255u) & ~size_t(255u); return o; };
    const std::vector<size_t> by_hand = {take((R + 1) * 4), take(ref_bytes), take(P * 4), take((P + 1) * 4), take(hap_bytes), take(P * 4), take(P * 4),
                                         take(hap_bytes * 2), take(ws_bytes), take(0), take(0), take(0), take(0)};
    const std::vector<size_t> in_numbers = {0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 6400, 6656, 6912, 7168};
    for (size_t i = 0; i < by_hand.size(); i++) expect("by_hand", i, by_hand[i], in_numbers[i]);
    expect("by_hand", 999, at, 7424);
    dd_align_batch db;
    dd_align_result dr;
    unsigned char *ws;
    int32_t *d_nev; dd_align_events *d_ev; dd_hap_variants_summary *d_sum; dd_hap_variant *d_va;
    const char src[64] = {0};                // a source changes nothing about the layout
    expect_layout("align", {arena_slot(&db.ref_off, (R + 1) * 4, src), arena_slot(&db.ref_seq, ref_bytes, src), arena_slot(&db.pair_ref, P * 4, src),
                            arena_slot(&db.hap_off, (P + 1) * 4, src), arena_slot(&db.hap_seq, hap_bytes, src), arena_slot(&dr.score, P * 4),
                            arena_slot(&dr.status, P * 4), arena_slot(&dr.ref_pos, hap_bytes * 2), arena_slot(&ws, ws_bytes), arena_slot(&d_nev, 0),
                            arena_slot(&d_ev, 0), arena_slot(&d_sum, 0), arena_slot(&d_va, 0)},
                  in_numbers, 7424);

    if (g_failed) return 1;
    std::printf("arena_layout_check: %d checks ok\n", g_checks);
    return 0;
}
