// pooled_vcf_capi.cpp — the extern "C" hooks of host/pooled_vcf.cpp and of pooledRealignedCigars (host/realigned_bam.cpp) for the pytest suite and dindel_tgi_amd/pooled_vcf.py (ctypes), in the pattern of vcf_candidates_capi.cpp.  Not part of the drop-in boundary.
#include <cstring>
#include <sstream>
#include <string>
#include "pooled_vcf.hpp"
#include "realigned_bam.hpp"

using namespace dindel;

static int emit(const std::string &s, char *out, int cap)
{
    if (int(s.size()) + 1 > cap) return -int(s.size()) - 1;
    memcpy(out, s.c_str(), s.size() + 1);
    return int(s.size());
}

// a JSON string of ASCII: every other byte as \u00XX, so that the text reaches Python byte for byte (pooled_vcf.py turns the Latin-1
// code points back into the bytes they stand for)
static void quoted(std::ostream &os, const std::string &s)
{
    static const char *const hex = "0123456789abcdef";
    os << '"';
    for (size_t i = 0; i < s.size(); i++) {
        const unsigned char c = (unsigned char)s[i];
        if (c == '"' || c == '\\') os << '\\' << s[i];
        else if (c < 0x20 || c >= 0x7f) os << "\\u00" << hex[c >> 4] << hex[c & 15];
        else os << s[i];
    }
    os << '"';
}

// the notes of the last conversion of this thread: a caller whose buffer was too small fetches them with ddh_pooled_last_notes
// instead of running the conversion again
static thread_local std::string lastNotes;

static int notes(const std::ostringstream &err, const std::ostringstream &so, bool threw, const std::string &thrown, char *out, int cap)
{
    std::ostringstream os;
    os << "{\"stderr\":";
    quoted(os, err.str());
    os << ",\"stdout\":";
    quoted(os, so.str());
    if (threw) { os << ",\"throw\":"; quoted(os, thrown); }
    os << "}";
    lastNotes = os.str();
    return emit(lastNotes, out, cap);
}
extern "C" int ddh_pooled_last_notes(char *out, int cap) { return emit(lastNotes, out, cap); }

// the tools' mains
extern "C" int ddh_pooled2vcf_main(int argc, char **argv) { return pooledVcfMain(argc, argv); }
extern "C" int ddh_pooled2glf_main(int argc, char **argv) { return pooledGlfMain(argc, argv); }

// processPooledGLFFiles on a list file: {"stderr":"...","stdout":"..."} and "throw":"..." where the script dies.  Returns the length written,
// or -(needed size) if cap is too small: the conversion has run then, and ddh_pooled_last_notes hands its notes over.
extern "C" int ddh_pooled_vcf_json(const char *listFile, const char *refFile, const char *outFile, int numSamples, int numBamFiles, int maxHPLen, int filterFR,
                                   int filterQual, char *out, int cap)
{
    std::ostringstream err, so;
    std::string thrown;
    bool threw = false;
    try {
        PooledVcfOptions o;
        o.outputFile = outFile; o.refFile = refFile; o.numSamples = numSamples; o.numBamFiles = numBamFiles; o.maxHPLen = maxHPLen; o.filterFR = filterFR != 0;
        o.filterQual = filterQual;
        processPooledGLFFiles(listFile, o, err, so);
    } catch (const std::string &e) { threw = true; thrown = e; }
    return notes(err, so, threw, thrown, out, cap);
}

// makeGLF on its three files and the output's name; the same JSON
extern "C" int ddh_pooled_glf_json(const char *glfList, const char *callFile, const char *outFile, const char *bamList, char *out, int cap)
{
    std::ostringstream err, so;
    std::string thrown;
    bool threw = false;
    try { makeGLF(glfList, outFile, callFile, bamList, err, so); } catch (const std::string &e) { threw = true; thrown = e; }
    return notes(err, so, threw, thrown, out, cap);
}

// Variant4 of any (REF, ALT): {"type":"snp","offset":2,"str":"A=>C"} or {"throw":"..."}
extern "C" int ddh_variant4_any_json(const char *ref, const char *alt, char *out, int cap)
{
    std::ostringstream os;
    try {
        const Variant4 v = variant4AnyLength(ref, alt);
        os << "{\"type\":\"" << v.type << "\",\"offset\":" << v.offset << ",\"str\":";
        quoted(os, v.str);
        os << "}";
    } catch (const std::string &e) { os.str(""); os << "{\"throw\":"; quoted(os, e); os << "}"; }
    lastNotes = os.str();
    return emit(lastNotes, out, cap);
}

// getPercentiles: depths[i] seen counts[i] times, the percentiles pct[0 .. np) -> outK[0 .. np)
extern "C" void ddh_get_percentiles(const long *depths, const long *counts, int n, const int *pct, int np, long *outK)
{
    std::map<long, long> hist;
    for (int i = 0; i < n; i++) hist[depths[i]] = counts[i];
    const std::vector<long> k = getPercentiles(hist, std::vector<int>(pct, pct + np));
    for (int i = 0; i < np; i++) outK[i] = k[size_t(i)];
}

// pooledRealignedCigars on hand-made likelihoods: ll[h * R + r], onHap[r].  Haplotype h lies on the reference at offset 10 h, base for
// base, and every read (readLen bases) lies on its haplotype from the haplotype's first base on — so getCIGAR gives readLen M at
// refSeqPos + 10 h, and refPos names the haplotype chosen.  numOps[r] and refPos[r] come back (0 and -1 for a read without onHap).
extern "C" int ddh_pooled_realigned_cigars(const double *ll, int H, int R, const int *onHap, int readLen, int refSeqPos, int *numOps, int *refPos)
{
    try {
        std::vector<CIGAR> cigars;
        pooledRealignedCigars(size_t(H), size_t(R), [&](size_t h, size_t r) { return ll[h * size_t(R) + r]; }, [&](size_t r) { return onHap[r] != 0; },
                              [&](size_t h, size_t) {
                                  std::vector<int> hapRefPos(size_t(readLen) + 4);
                                  for (size_t i = 0; i < hapRefPos.size(); i++) hapRefPos[i] = int(10 * h + i);
                                  MLAlignment ml;
                                  for (int b = 0; b < readLen; b++) ml.hpos.push_back(b);
                                  return getCIGAR(hapRefPos, hapRefPos.size(), ml, size_t(readLen), refSeqPos);
                              }, cigars);
        for (int r = 0; r < R; r++) { numOps[r] = int(cigars[size_t(r)].size()); refPos[r] = cigars[size_t(r)].refPos; }
        return 0;
    } catch (const std::string &) { return -1; }
}
