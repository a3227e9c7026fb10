// vcf_candidates_capi.cpp — the extern "C" hooks of host/vcf_candidates.cpp and of the discovery stage with known sites (host/discover.cpp)
// for the pytest suite and dindel_tgi_amd/vcf_candidates.py (ctypes), in the pattern of windows_capi.cpp.  Not part of the drop-in boundary.
#include <cstring>
#include <sstream>
#include <string>
#include "discover.hpp"

using namespace dindel;

static int emit(const std::string &s, char *out, int cap)
{
    if (int(s.size()) + 1 > cap) return -int(s.size()) - 1;
    memcpy(out, s.c_str(), s.size() + 1);
    return int(s.size());
}

static void quoted(std::ostream &os, const std::string &s)
{
    os << '"';
    for (size_t i = 0; i < s.size(); i++) {
        const unsigned char c = (unsigned char)s[i];
        if (c == '"' || c == '\\') os << '\\' << s[i];
        else if (c == '\n') os << "\\n";
        else if (c == '\t') os << "\\t";
        else if (c < 0x20 || c >= 0x7f) os << ' ';
        else os << s[i];
    }
    os << '"';
}

// the tool's main
extern "C" int ddh_vcf2candidates_main(int argc, char **argv) { return vcfCandidatesMain(argc, argv); }

// Variant4 of one (REF, ALT) of unequal lengths: {"type":"ins","offset":1,"str":"+TT"} or {"throw":"..."}
extern "C" int ddh_variant4_json(const char *ref, const char *alt, char *out, int cap)
{
    std::ostringstream os;
    try {
        const Variant4 v = variant4(ref, alt);
        os << "{\"type\":\"" << v.type << "\",\"offset\":" << v.offset << ",\"str\":";
        quoted(os, v.str);
        os << "}";
    } catch (const std::string &e) { os.str(""); os << "{\"throw\":"; quoted(os, e); os << "}"; }
    return emit(os.str(), out, cap);
}

// The conversion of the comma-separated VCFs to outFile (tid and region NULL or both given): {"lines":N,"stderr":"...","stdout":"..."} and
// "throw":"..." where the script dies.  Returns the length written, or -(needed size) if cap is too small (the conversion has run then).
extern "C" int ddh_vcf_convert_json(const char *vcfFiles, const char *refFile, const char *outFile, double minQual, const char *tid, const char *region,
                                    char *out, int cap)
{
    std::ostringstream err, so, os;
    std::string thrown;
    bool threw = false;
    long n = 0;
    try {
        VcfConvertOptions o;
        o.inputFiles = vcfFiles; o.refFile = refFile; o.outputFile = outFile; o.minQual = minQual;
        if (tid && region) { o.haveRegion = true; o.tid = tid; parseRegion(region, o.start, o.end); }
        n = convertVcfToCandidates(o, err, so);
    } catch (const std::string &e) { threw = true; thrown = e; }
    os << "{\"lines\":" << n << ",\"stderr\":";
    quoted(os, err.str());
    os << ",\"stdout\":";
    quoted(os, so.str());
    if (threw) { os << ",\"throw\":"; quoted(os, thrown); }
    os << "}";
    return emit(os.str(), out, cap);
}

// ddh_discover_windows (windows_capi.cpp) with the known sites of dindel_gpu --discover --candidateVCF: candidateVCF the comma-separated
// list, vcfOnly != 0 for --vcfCandidatesOnly.  Returns the number of window lines, or -1 with the message in err.
extern "C" long ddh_discover_windows_vcf(const char *bamFile, const char *bamList, const char *tid, const char *region, const char *refFile,
                                         const char *outputPrefix, const char *candidateVCF, double minQual, int vcfOnly, long minDist, long minCount,
                                         long maxCount, int batchCandidates, int eventsCap, int hostConvert, AlignHook hook, void *data, char *err, int cap)
{
    try {
        DiscoverOptions o;
        if (bamFile && *bamFile) o.bamFiles.push_back(bamFile);
        else if (bamList && *bamList) o.bamFiles = readBamList(bamList);
        if (tid && region) { o.haveRegion = true; o.tid = tid; parseRegion(region, o.start, o.end); }
        o.refFile = refFile; o.outputPrefix = outputPrefix;
        if (candidateVCF) o.candidateVCF = candidateVCF;
        o.minQual = minQual; o.vcfCandidatesOnly = vcfOnly != 0;
        o.minDist = minDist;
        o.filter = minCount >= 0 || maxCount >= 0;
        if (minCount >= 0) o.minCount = minCount;
        if (maxCount >= 0) o.maxCount = maxCount;
        o.candidates.quiet = true;
        o.candidates.hostConvert = hostConvert != 0;
        if (batchCandidates > 0) o.candidates.batchCandidates = batchCandidates;
        if (eventsCap > 0) o.candidates.eventsCap = eventsCap;
        o.candidates.hook = hook; o.candidates.hookData = data;
        CandidateStats stats;
        return discoverWindows(o, stats);
    } catch (const std::string &e) {
        if (err && cap > 0) emit(e.substr(0, size_t(cap - 1)), err, cap);
        return -1;
    }
}
