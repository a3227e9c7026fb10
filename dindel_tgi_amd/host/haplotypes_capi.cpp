// haplotypes_capi.cpp — the extern "C" hooks of host/haplotypes.cpp for the pytest suite (ctypes), in the pattern of candidates_capi.cpp.
// Not part of the drop-in boundary.  Strings travel as hex so that no byte needs escaping.
#include <cstring>
#include <sstream>
#include <string>
#include "haplotypes.hpp"

using namespace dindel;

namespace {

int emit(const std::string &s, char *out, int cap)
{
    if (int(s.size()) + 1 > cap) return -int(s.size()) - 1;
    memcpy(out, s.c_str(), s.size() + 1);
    return int(s.size());
}

std::string hex(const std::string &s)
{
    static const char *d = "0123456789abcdef";
    std::string o;
    for (size_t i = 0; i < s.size(); i++) { o += d[(unsigned char)s[i] >> 4]; o += d[s[i] & 15]; }
    return o;
}

std::string unhex(const std::string &s)
{
    std::string o;
    for (size_t i = 0; i + 1 < s.size(); i += 2) o += char(strtol(s.substr(i, 2).c_str(), NULL, 16));
    return o;
}

void blockJson(std::ostream &os, const HapBlockTable &hb, long origin)
{
    os << "[" << long(hb.start) - origin << "," << (hb.insertion ? 0 : long(hb.end) - long(hb.start) + 1) << ",[";
    for (size_t i = 0; i < hb.entries.size(); i++)
        os << (i ? "," : "") << "[\"" << hex(hb.entries[i].seq) << "\"," << hb.entries[i].count << "," << (hb.entries[i].isRef ? "true" : "false") << "]";
    os << "]]";
}

std::string tableJson(const WindowTable &t, long rs)
{
    std::ostringstream os;
    os << "\"blocks\":[";
    for (size_t k = 0; k < t.blocks.size(); k++) { if (k) os << ","; blockJson(os, t.blocks[k], rs); }
    os << "],\"ins\":[";
    for (size_t k = 0; k < t.insertions.size(); k++) { if (k) os << ","; blockJson(os, t.insertions[k], rs); }
    os << "],\"left\":" << t.left;
    return os.str();
}

// "B start end insertion" lines, each followed by its "E hexseq count isRef freq" lines ("-" = the empty string)
std::vector<HapBlockTable> parseBlocks(const char *text)
{
    std::vector<HapBlockTable> v;
    std::istringstream in(text ? text : "");
    std::string tag;
    while (in >> tag) {
        if (tag == "B") { HapBlockTable hb; int ins; in >> hb.start >> hb.end >> ins; hb.insertion = ins != 0; v.push_back(hb); }
        else if (tag == "E" && !v.empty()) {
            BlockEntry e; std::string h; int isRef;
            in >> h >> e.count >> isRef >> e.freq;
            e.seq = h == "-" ? std::string() : unhex(h); e.isRef = isRef != 0;
            v.back().entries.push_back(e);
        }
    }
    return v;
}

// "pos string addComb" lines
std::vector<AlignedVariant> parseVariants(const char *text)
{
    std::vector<AlignedVariant> v;
    std::istringstream in(text ? text : "");
    int pos, comb; std::string s;
    while (in >> pos >> s >> comb) v.push_back(AlignedVariant(s, pos, -1.0, comb != 0));
    return v;
}

} // namespace

extern "C" int ddh_haplotypes_main(int argc, char **argv) { return haplotypesMain(argc, argv); }

// blockTableHost into the caller's flat tables (sized by dd_hap_blocks_offsets or by hand)
extern "C" void ddh_hap_block_table_flat(const dd_hap_batch *b, dd_hap_blocks *t) { blockTableHost(*b, *t); }

// window w of the batch as a table: mode 0 = blockTableHost + tableFromFlat ({"status":s} alone when the window is not OK),
// mode 1 = sequentialTable ({"throw":"..."} when it throws)
extern "C" int ddh_hap_window_table_json(const dd_hap_batch *b, int w, int mode, char *out, int cap)
{
    std::ostringstream os;
    try {
        if (mode == 0) {
            HapTablesData store;
            store.size(*b);
            dd_hap_blocks t = store.tables();
            blockTableHost(*b, t);
            os << "{\"status\":" << t.status[w];
            if (t.status[w] == DD_HAPDIST_OK) os << "," << tableJson(tableFromFlat(*b, t, w), b->win_rs[w]);
            os << "}";
        } else os << "{" << tableJson(sequentialTable(*b, w), b->win_rs[w]) << "}";
    } catch (std::string &e) { os.str(""); os << "{\"throw\":\"" << e << "\"}"; }
    return emit(os.str(), out, cap);
}

// an OK window of flat tables that came from somewhere else (the device) through tableFromFlat
extern "C" int ddh_hap_table_from_flat_json(const dd_hap_batch *b, const dd_hap_blocks *t, int w, char *out, int cap)
{
    std::ostringstream os;
    try { os << "{" << tableJson(tableFromFlat(*b, *t, w), b->win_rs[w]) << "}"; }
    catch (std::string &e) { os.str(""); os << "{\"throw\":\"" << e << "\"}"; }
    return emit(os.str(), out, cap);
}

// setThresholds on blocks given as text: {"logNumHap":x,"blocks":[...]} (positions absolute) or {"throw":...}
extern "C" int ddh_hap_thresholds_json(const char *blocks, int maxHap, char *out, int cap)
{
    std::ostringstream os;
    try {
        std::vector<HapBlockTable> hbs = parseBlocks(blocks);
        const double logNum = setThresholds(hbs, size_t(maxHap));
        os.precision(17);
        os << "{\"logNumHap\":" << logNum << ",\"blocks\":[";
        for (size_t k = 0; k < hbs.size(); k++) { if (k) os << ","; blockJson(os, hbs[k], 0); }
        os << "]}";
    } catch (std::string &e) { os.str(""); os << "{\"throw\":\"" << e << "\"}"; }
    return emit(os.str(), out, cap);
}

// generateHaplotypes on blocks and variants given as text: {"haps":["hex",...]} or {"throw":...}
extern "C" int ddh_hap_generate_json(const char *blocks, const char *variants, int changeINStoN, char *out, int cap)
{
    std::ostringstream os;
    try {
        const std::vector<std::string> haps = generateHaplotypes(parseBlocks(blocks), parseVariants(variants), changeINStoN != 0);
        os << "{\"haps\":[";
        for (size_t h = 0; h < haps.size(); h++) os << (h ? "," : "") << "\"" << hex(haps[h]) << "\"";
        os << "]}";
    } catch (std::string &e) { os.str(""); os << "{\"throw\":\"" << e << "\"}"; }
    return emit(os.str(), out, cap);
}

// one window end to end on the host: mode 0 = closed form (sequentialTable when its status is not OK), mode 1 = sequentialTable.
// {"left":l,"right":r,"haps":[...]} or {"message":"..."}
extern "C" int ddh_hap_window_haplotypes_json(const dd_hap_batch *b, int w, int mode, unsigned left, unsigned right, const char *variants,
                                              int nReads, int maxHap, int skipMaxHap, double maxHapReadProd, int changeINStoN, char *out, int cap)
{
    std::ostringstream os;
    WindowCandidates win;
    win.leftPos = left; win.rightPos = right; win.nReads = size_t(nReads);
    HaplotypeOptions opt;
    opt.maxHap = size_t(maxHap); opt.skipMaxHap = size_t(skipMaxHap); opt.maxHapReadProd = maxHapReadProd; opt.changeINStoN = changeINStoN != 0;
    try {
        win.variants = parseVariants(variants);
        WindowTable table;
        bool have = false;
        if (mode == 0) {
            HapTablesData store;
            store.size(*b);
            dd_hap_blocks t = store.tables();
            blockTableHost(*b, t);
            if (t.status[w] == DD_HAPDIST_OK) { table = tableFromFlat(*b, t, w); have = true; }
        }
        if (!have) table = sequentialTable(*b, w);
        haplotypesFromTable(table, uint32_t(b->win_rs[w]), opt, win);
    } catch (std::string &e) { win.haps.clear(); win.message = e; }
    if (!win.message.empty()) os << "{\"message\":\"" << win.message << "\"}";
    else {
        os << "{\"left\":" << win.leftPos << ",\"right\":" << win.rightPos << ",\"haps\":[";
        for (size_t h = 0; h < win.haps.size(); h++) os << (h ? "," : "") << "\"" << hex(win.haps[h]) << "\"";
        os << "]}";
    }
    return emit(os.str(), out, cap);
}
