// windows_capi.cpp — the extern "C" hooks of host/windows.cpp and host/discover.cpp for the pytest suite and dindel_tgi_amd/windows.py
// (ctypes), in the pattern of candidates_capi.cpp.  Not part of the drop-in boundary.
#include <cstring>
#include <iostream>
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
        else if (c < 0x20) os << ' ';
        else os << s[i];
    }
    os << '"';
}

static std::vector<std::string> splitLines(const char *text)
{
    std::vector<std::string> lines;
    std::istringstream is(text ? text : "");
    std::string line;
    while (std::getline(is, line)) lines.push_back(line);
    return lines;
}

// the tool's main
extern "C" int ddh_windows_main(int argc, char **argv) { return windowsMain(argc, argv); }

// makeWindows over the lines of `text` (filter != 0: selectCandidates first): {"files":[{"number":N,"lines":[...]},...],"selected":[...],
// "stderr":"..."} and "throw":"..." if it threw.  Returns the length written, or -(needed size) if cap is too small.
extern "C" int ddh_make_windows_json(const char *text, long minDist, long numWindowsPerFile, int filter, long minCount, long maxCount, char *out, int cap)
{
    std::ostringstream err, os;
    std::vector<WindowFile> files;
    std::vector<std::string> lines = splitLines(text), selected;
    std::string thrown;
    bool threw = false;
    try {
        if (filter) lines = selected = selectCandidates(lines, minCount, maxCount, err);
        makeWindows(lines, minDist, numWindowsPerFile, files, err);
    } catch (const std::string &e) { threw = true; thrown = e; }
    os << "{\"files\":[";
    for (size_t f = 0; f < files.size(); f++) {
        os << (f ? "," : "") << "{\"number\":" << files[f].number << ",\"lines\":[";
        for (size_t l = 0; l < files[f].lines.size(); l++) { os << (l ? "," : ""); quoted(os, files[f].lines[l]); }
        os << "]}";
    }
    os << "],\"selected\":[";
    for (size_t l = 0; l < selected.size(); l++) { os << (l ? "," : ""); quoted(os, selected[l]); }
    os << "],\"stderr\":";
    quoted(os, err.str());
    if (threw) { os << ",\"throw\":"; quoted(os, thrown); }
    os << "}";
    return emit(os.str(), out, cap);
}

// selectCandidates alone: {"selected":[...],"stderr":"..."} and "throw":"..." if it threw
extern "C" int ddh_select_candidates_json(const char *text, long minCount, long maxCount, char *out, int cap)
{
    std::ostringstream err, os;
    std::vector<std::string> selected;
    std::string thrown;
    bool threw = false;
    try { selected = selectCandidates(splitLines(text), minCount, maxCount, err); } catch (const std::string &e) { threw = true; thrown = e; }
    os << "{\"selected\":[";
    for (size_t l = 0; l < selected.size(); l++) { os << (l ? "," : ""); quoted(os, selected[l]); }
    os << "],\"stderr\":";
    quoted(os, err.str());
    if (threw) { os << ",\"throw\":"; quoted(os, thrown); }
    os << "}";
    return emit(os.str(), out, cap);
}

// clusterKeys: keys[n] of the n sorted distinct positions
extern "C" void ddh_cluster_keys(const long *positions, int n, long minDist, long *keys)
{
    const std::vector<long> k = clusterKeys(std::vector<long>(positions, positions + n), minDist);
    for (int i = 0; i < n; i++) keys[i] = k[size_t(i)];
}

// The discovery stage of dindel_gpu --discover with an aligner in place of the device (NULL = the device).  bamFile or bamList; tid and
// region NULL or both given; minCount / maxCount < 0: not given (given one, the other takes the script's default).  Returns the number of
// window lines, or -1 with the message in err.
extern "C" long ddh_discover_windows(const char *bamFile, const char *bamList, const char *tid, const char *region, const char *refFile, const char *outputPrefix,
                                     long minDist, long minCount, long maxCount, int batchCandidates, int eventsCap, int hostConvert,
                                     AlignHook hook, void *data, char *err, int cap)
{
    try {
        DiscoverOptions o;
        if (bamFile && *bamFile) o.bamFiles.push_back(bamFile);
        else if (bamList && *bamList) o.bamFiles = readBamList(bamList);
        if (tid && region) { o.haveRegion = true; o.tid = tid; parseRegion(region, o.start, o.end); }
        o.refFile = refFile; o.outputPrefix = outputPrefix;
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
