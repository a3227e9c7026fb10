// align_capi.cpp — the extern "C" hook of host/align_haplotypes.cpp for the pytest suite (ctypes), in the pattern of host_capi.cpp's
// ddh_*_json functions.  A file of its own so that host_capi.cpp keeps building without align_haplotypes.cpp (tests/sanitize_cpu.sh names
// its sources one by one).  Not part of the drop-in boundary.
#include <cstring>
#include <sstream>
#include <string>
#include "align_haplotypes.hpp"
#include "../../include/dindel_hmm.h"

using namespace dindel;

static int emit(const std::string &s, char *out, int cap)
{
    if (int(s.size()) + 1 > cap) return -int(s.size()) - 1;
    memcpy(out, s.c_str(), s.size() + 1);
    return int(s.size());
}

// alignHaplotypes + the end of getHaplotypes for one window (host/align_haplotypes.hpp).  ref / haps: raw bytes with their lengths (the
// haplotypes back to back).  ref_pos: the alignments, one entry per haplotype base (dd_align_result.ref_pos), or NULL: align on `device`.
// Out: {"kept":[{"index":i,"align":"...","refHpos":[...],"indels":[[key,"string",startHap,endHap,startRead,endRead,leftFlankHap,
// rightFlankHap,leftFlankRead,rightFlankRead],...],"snps":[...]},...]} with i the haplotype's index as it came in, or {"throw":"..."}.
extern "C" int ddh_align_haplotypes_json(const char *ref, int ref_len, const char *haps, const int *hap_len, int n_haps, const int *ref_pos,
                                         int device, char *out, int cap)
{
    try {
        const std::string refSeq(ref, size_t(ref_len));
        WindowHaplotypes w;
        w.index = 0; w.leftPos = 0; w.rightPos = 0;
        std::vector<std::vector<int> > pos(size_t(n_haps > 0 ? n_haps : 0));
        size_t at = 0;
        for (int h = 0; h < n_haps; h++) {
            w.haps.push_back(Haplotype(std::string(haps + at, size_t(hap_len[h]))));
            if (ref_pos) pos[size_t(h)].assign(ref_pos + at, ref_pos + at + hap_len[h]);
            at += size_t(hap_len[h]);
        }
        std::vector<int> kept;
        if (ref_pos) finishWindowHaplotypes(w, refSeq, pos, &kept);
        else {
            // through the batch entry; the kept haplotypes' indices are recovered by matching their sequences in order
            std::vector<WindowHaplotypes> wins(1, w);
            alignHaplotypesBatch(wins, std::vector<std::string>(1, refSeq), device);
            std::vector<Haplotype> all = w.haps;
            size_t k = 0;
            for (size_t h = 0; h < all.size() && k < wins[0].haps.size(); h++)
                if (all[h].seq == wins[0].haps[k].seq) { kept.push_back(int(h)); k++; }
            w = wins[0];
        }
        std::ostringstream os;
        os << "{\"kept\":[";
        for (size_t h = 0; h < w.haps.size(); h++) {
            const Haplotype &hap = w.haps[h];
            os << (h ? "," : "") << "{\"index\":" << (h < kept.size() ? kept[h] : -1) << ",\"align\":\"" << hap.align << "\",\"refHpos\":[";
            for (size_t b = 0; b < hap.refHpos.size(); b++) os << (b ? "," : "") << hap.refHpos[b];
            os << "]";
            for (int pass = 0; pass < 2; pass++) {
                const std::map<int, AlignedVariant> &m = pass ? hap.snps : hap.indels;
                os << (pass ? ",\"snps\":[" : ",\"indels\":[");
                bool first = true;
                for (std::map<int, AlignedVariant>::const_iterator it = m.begin(); it != m.end(); ++it, first = false) {
                    const AlignedVariant &v = it->second;
                    os << (first ? "" : ",") << "[" << it->first << ",\"" << v.getString() << "\"," << v.getStartHap() << "," << v.getEndHap() << ","
                       << v.getStartRead() << "," << v.getEndRead() << "," << v.getLeftFlankHap() << "," << v.getRightFlankHap() << ","
                       << v.getLeftFlankRead() << "," << v.getRightFlankRead() << "]";
                }
                os << "]";
            }
            os << "}";
        }
        os << "]}";
        return emit(os.str(), out, cap);
    } catch (std::string &e) {
        return emit(std::string("{\"throw\":\"") + e + "\"}", out, cap);
    }
}

// The variants kernel's twin and the records-to-Haplotype step against the string walk, for one window (host/align_haplotypes.hpp).
// Inputs as ddh_align_haplotypes_json, ref_pos required (int16 values in ints).  summary [n_haps * 4] and variants [n_haps * cap * 8]
// (int32 / int16, may be NULL) receive hapVariantsHost's output.  Out: {"records":W,"strings":W} with W a window as
// ddh_align_haplotypes_json prints it: through finishWindowHaplotypesFromVariants and through finishWindowHaplotypes; plus
// "firstLast":[[firstBase,lastBase],...] of convertHaplotypeAlignment per haplotype.
static void printWindow(std::ostream &os, const WindowHaplotypes &w, const std::vector<int> &kept)
{
    os << "{\"kept\":[";
    for (size_t h = 0; h < w.haps.size(); h++) {
        const Haplotype &hap = w.haps[h];
        os << (h ? "," : "") << "{\"index\":" << (h < kept.size() ? kept[h] : -1) << ",\"align\":\"" << hap.align << "\",\"refHpos\":[";
        for (size_t b = 0; b < hap.refHpos.size(); b++) os << (b ? "," : "") << hap.refHpos[b];
        os << "]";
        for (int pass = 0; pass < 2; pass++) {
            const std::map<int, AlignedVariant> &m = pass ? hap.snps : hap.indels;
            os << (pass ? ",\"snps\":[" : ",\"indels\":[");
            bool first = true;
            for (std::map<int, AlignedVariant>::const_iterator it = m.begin(); it != m.end(); ++it, first = false) {
                const AlignedVariant &v = it->second;
                os << (first ? "" : ",") << "[" << it->first << ",\"" << v.getString() << "\"," << v.getStartHap() << "," << v.getEndHap() << ","
                   << v.getStartRead() << "," << v.getEndRead() << "," << v.getLeftFlankHap() << "," << v.getRightFlankHap() << ","
                   << v.getLeftFlankRead() << "," << v.getRightFlankRead() << "]";
            }
            os << "]";
        }
        os << "}";
    }
    os << "]}";
}

extern "C" int ddh_hap_variants_json(const char *ref, int ref_len, const char *haps, const int *hap_len, int n_haps, const int *ref_pos, int cap,
                                     int32_t *summary, int16_t *variants, char *out, int out_cap)
{
    try {
        const std::string refSeq(ref, size_t(ref_len));
        WindowHaplotypes w;
        w.index = 0; w.leftPos = 0; w.rightPos = 0;
        const size_t nH = n_haps > 0 ? size_t(n_haps) : 0;
        std::vector<std::vector<int> > pos(nH);
        std::vector<int32_t> refOff(2, 0), hapOff(1, 0), pairRef(nH, 0), status(nH, DD_ALIGN_OK);
        refOff[1] = ref_len;
        std::vector<int16_t> slice;
        size_t at = 0;
        for (int h = 0; h < n_haps; h++) {
            w.haps.push_back(Haplotype(std::string(haps + at, size_t(hap_len[h]))));
            pos[size_t(h)].assign(ref_pos + at, ref_pos + at + hap_len[h]);
            for (int b = 0; b < hap_len[h]; b++) slice.push_back(int16_t(ref_pos[at + size_t(b)]));
            at += size_t(hap_len[h]);
            hapOff.push_back(int32_t(at));
        }
        dd_align_batch b;
        b.n_refs = 1; b.ref_off = refOff.data(); b.ref_seq = ref; b.n_pairs = n_haps; b.pair_ref = pairRef.data(); b.hap_off = hapOff.data(); b.hap_seq = haps;
        std::vector<dd_hap_variants_summary> sum(nH);
        std::vector<dd_hap_variant> var(nH * size_t(cap));
        memset(var.data(), 0, var.size() * sizeof(dd_hap_variant));
        hapVariantsHost(b, status.data(), slice.data(), sum.data(), var.data(), cap);
        if (summary) memcpy(summary, sum.data(), sum.size() * sizeof(dd_hap_variants_summary));
        if (variants) memcpy(variants, var.data(), var.size() * sizeof(dd_hap_variant));
        std::vector<const int16_t *> slices;
        for (int h = 0; h < n_haps; h++) slices.push_back(slice.data() + hapOff[size_t(h)]);
        std::ostringstream os;
        os << "{\"firstLast\":[";
        for (int h = 0; h < n_haps; h++) {
            Haplotype tmp(w.haps[size_t(h)].seq);
            int fb = 0, lb = 0;
            convertHaplotypeAlignment(refSeq, tmp, pos[size_t(h)], &fb, &lb);
            os << (h ? "," : "") << "[" << fb << "," << lb << "]";
        }
        WindowHaplotypes a = w, c = w;
        std::vector<int> keptA, keptC;
        finishWindowHaplotypesFromVariants(a, refSeq, sum.data(), var.data(), cap, slices, &keptA);
        finishWindowHaplotypes(c, refSeq, pos, &keptC);
        os << "],\"records\":";
        printWindow(os, a, keptA);
        os << ",\"strings\":";
        printWindow(os, c, keptC);
        os << "}";
        return emit(os.str(), out, out_cap);
    } catch (std::string &e) {
        return emit(std::string("{\"throw\":\"") + e + "\"}", out, out_cap);
    }
}
