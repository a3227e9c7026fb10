// hap_variants_check.cpp — a stand-alone check of host/align_haplotypes.cpp's record path for a sanitizer build (no Python, no GPU):
//   g++ -std=c++11 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include tests/hap_variants_check.cpp
//       dindel_tgi_amd/host/align_haplotypes.cpp -o hap_variants_check && ./hap_variants_check
// hapVariantsHost + finishWindowHaplotypesFromVariants against convertHaplotypeAlignment + finishWindowHaplotypes on hand-written gapped
// rows and on generated ones (repeats, runs to both ends, overhangs, long insertions, caps of 1 and 16), field for field.  The device
// entries alignHaplotypesBatch would call are stubbed: nothing here reaches them.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../dindel_tgi_amd/host/align_haplotypes.hpp"

extern "C" {
int dd_align_haplotypes(const dd_align_batch *, dd_align_result *, int) { return DD_ERR_NO_DEVICE; }
int dd_align_haplotypes_variants(const dd_align_batch *, dd_align_result *, dd_hap_variants_summary *, dd_hap_variant *, int, int) { return DD_ERR_NO_DEVICE; }
const char *dd_last_error(void) { return "stub"; }
}

using namespace dindel;

namespace {

struct Case { std::string ref, hap; std::vector<int> pos; };

Case fromRows(const std::string &row0, const std::string &row1)
{
    Case c;
    int i = 0;
    for (size_t k = 0; k < row0.size(); k++) {
        if (row1[k] != '-') { c.hap += row1[k]; c.pos.push_back(row0[k] != '-' ? i : -1 - i); }
        if (row0[k] != '-') { c.ref += row0[k]; i++; }
    }
    return c;
}

bool sameVariants(const std::map<int, AlignedVariant> &a, const std::map<int, AlignedVariant> &b)
{
    if (a.size() != b.size()) return false;
    std::map<int, AlignedVariant>::const_iterator x = a.begin(), y = b.begin();
    for (; x != a.end(); ++x, ++y) {
        const AlignedVariant &u = x->second, &v = y->second;
        if (x->first != y->first || u.getString() != v.getString() || u.getStartHap() != v.getStartHap() || u.getEndHap() != v.getEndHap() ||
            u.getStartRead() != v.getStartRead() || u.getEndRead() != v.getEndRead() || u.getLeftFlankHap() != v.getLeftFlankHap() ||
            u.getRightFlankHap() != v.getRightFlankHap() || u.getLeftFlankRead() != v.getLeftFlankRead() || u.getRightFlankRead() != v.getRightFlankRead())
            return false;
    }
    return true;
}

unsigned long long g_state = 88172645463325252ull;
unsigned rnd(unsigned n) { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return unsigned(g_state % n); }

// one window of haplotypes that share `ref`; false: a difference
bool checkWindow(const std::string &ref, const std::vector<Case> &cs, int cap)
{
    WindowHaplotypes a, b;
    a.index = b.index = 0; a.leftPos = b.leftPos = 0; a.rightPos = b.rightPos = 0;
    std::vector<std::vector<int> > pos;
    std::vector<int32_t> refOff(2, 0), hapOff(1, 0), pairRef(cs.size(), 0), status(cs.size(), DD_ALIGN_OK);
    refOff[1] = int32_t(ref.size());
    std::string hapAll;
    std::vector<int16_t> slice;
    for (size_t h = 0; h < cs.size(); h++) {
        a.haps.push_back(Haplotype(cs[h].hap)); b.haps.push_back(Haplotype(cs[h].hap));
        pos.push_back(cs[h].pos);
        hapAll += cs[h].hap;
        for (size_t k = 0; k < cs[h].pos.size(); k++) slice.push_back(int16_t(cs[h].pos[k]));
        hapOff.push_back(int32_t(hapAll.size()));
    }
    dd_align_batch B;
    B.n_refs = 1; B.ref_off = refOff.data(); B.ref_seq = ref.data(); B.n_pairs = int32_t(cs.size()); B.pair_ref = pairRef.data();
    B.hap_off = hapOff.data(); B.hap_seq = hapAll.data();
    // exactly-sized arrays: a record or a summary written past its slice is the sanitizer's to find
    std::vector<dd_hap_variants_summary> sum(cs.size());
    std::vector<dd_hap_variant> var(cs.size() * size_t(cap));
    hapVariantsHost(B, status.data(), slice.data(), sum.data(), var.data(), cap);
    std::vector<const int16_t *> slices;
    for (size_t h = 0; h < cs.size(); h++) slices.push_back(slice.data() + hapOff[h]);
    std::vector<int> keptA, keptB;
    finishWindowHaplotypesFromVariants(a, ref, sum.data(), var.data(), cap, slices, &keptA);
    finishWindowHaplotypes(b, ref, pos, &keptB);
    if (keptA != keptB || a.haps.size() != b.haps.size()) return false;
    for (size_t h = 0; h < a.haps.size(); h++)
        if (a.haps[h].seq != b.haps[h].seq || a.haps[h].align != b.haps[h].align || a.haps[h].refHpos != b.haps[h].refHpos ||
            !sameVariants(a.haps[h].indels, b.haps[h].indels) || !sameVariants(a.haps[h].snps, b.haps[h].snps)) return false;
    return true;
}

} // namespace

int main()
{
    static const char *const rows[][2] = {
        {"CAAAAT", "C-AAAT"}, {"AAAAT", "A-AAT"}, {"TCAAAA", "TCAA-A"}, {"GACACACT", "GAC--ACT"}, {"CAGCAGCAG", "C---AGCAG"}, {"CAAA-T", "CAAAAT"},
        {"A-AAA", "AAAAA"}, {"AC--ACT", "ACACACT"}, {"C---AGCAG", "CAGCAGCAG"}, {"ACGT", "CCGT"}, {"ACGT", "ACGA"}, {"A", "C"}, {"ACGT", "--G-"},
        {"ACnNTuAC", "AC-NTTAC"}, {"ACu-TAC", "ACuTTAC"}, {"AC--GTAC", "ACTT--AC"}, {"GT--ACGT", "--TTACGT"}, {"ACGT--AC", "AC--TTAC"}, {"ACGT--", "AC--TT"},
        {"--ACGT", "TTACGT"}, {"ACGT--", "ACGTTT"}, {"AACGT", "--CGT"}, {"AAC-GT", "--CTGT"}, {"A---C", "ATTTC"}, {"A--C", "ATTC"}};
    int n = 0, bad = 0;
    for (size_t k = 0; k < sizeof(rows) / sizeof(*rows); k++)
        for (int cap = 1; cap <= 16; cap += 15) {
            const Case c = fromRows(rows[k][0], rows[k][1]);
            n++;
            if (!checkWindow(c.ref, std::vector<Case>(1, c), cap)) { bad++; fprintf(stderr, "differs: %s / %s cap %d\n", rows[k][0], rows[k][1], cap); }
        }
    // generated: a reference from a short repeat unit or random letters, four haplotypes per window, each with up to three events
    for (int w = 0; w < 400; w++) {
        const int L = 1 + int(rnd(w % 4 ? 40 : 300)), unit = 1 + int(rnd(3));
        std::string ref;
        for (int i = 0; i < L; i++) ref += (w % 2) ? "ACGT"[(i % unit + w) % 4] : "ACGTNacu"[rnd(w % 5 ? 4 : 8)];
        std::vector<Case> cs;
        for (int h = 0; h < 4; h++) {
            std::string row0 = ref, row1 = ref;
            for (int e = int(rnd(4)); e > 0; e--) {
                const size_t at = rnd(unsigned(row0.size()) + 1);
                const unsigned kind = rnd(3), len = 1 + rnd(3);
                if (kind == 0 && at < row0.size() && row1[at] != '-' && row0[at] != '-') row1[at] = "ACGT"[rnd(4)];
                else if (kind == 1) { row0.insert(at, std::string(len, '-')); std::string ins; for (unsigned i = 0; i < len; i++) ins += "ACGT"[rnd(4)]; row1.insert(at, ins); }
                else for (size_t i = at; i < at + len && i < row1.size(); i++) if (row0[i] != '-' && row1[i] != '-') row1[i] = '-';
            }
            std::string r0, r1;                                  // no column of two gaps
            for (size_t i = 0; i < row0.size(); i++) if (row0[i] != '-' || row1[i] != '-') { r0 += row0[i]; r1 += row1[i]; }
            const Case c = fromRows(r0, r1);
            if (!c.hap.empty()) cs.push_back(c);
        }
        if (cs.empty()) continue;
        for (int cap = 1; cap <= 16; cap += 15) { n++; if (!checkWindow(ref, cs, cap)) { bad++; fprintf(stderr, "differs: generated window %d cap %d\n", w, cap); } }
    }
    printf("hap_variants_check: %d windows, %d differ\n", n, bad);
    return bad ? 1 : 0;
}
