// candidates_capi.cpp — the extern "C" hooks of host/candidates.cpp for the pytest suite (ctypes), in the pattern of align_capi.cpp.  Not
// part of the drop-in boundary.
#include <cstring>
#include <sstream>
#include <string>
#include "candidates.hpp"

using namespace dindel;

static int emit(const std::string &s, char *out, int cap)
{
    if (int(s.size()) + 1 > cap) return -int(s.size()) - 1;
    memcpy(out, s.c_str(), s.size() + 1);
    return int(s.size());
}

// the tool's main with an aligner in place of the device (NULL = the device): hook(data, host batch, status out, slices out)
extern "C" int ddh_candidates_main(int argc, char **argv, AlignHook hook, void *data) { return candidatesMain(argc, argv, hook, data); }

// alignmentEvents: the events of one slice; up to cap records of {kind, ref, len, hap} go to out, the true count is returned
extern "C" int ddh_alignment_events(const int16_t *refPos, int hapLen, int refLen, int16_t *out, int cap)
{
    std::vector<dd_align_events> ev;
    alignmentEvents(refPos, hapLen, refLen, ev);
    for (size_t k = 0; k < ev.size() && int(k) < cap; k++) { out[4 * k] = ev[k].kind; out[4 * k + 1] = ev[k].ref; out[4 * k + 2] = ev[k].len; out[4 * k + 3] = ev[k].hap; }
    return int(ev.size());
}

// cigarIndels of one record (its bytes without the length word): {"indels":[[refpos,len,"seq"],...]} and "throw":"..." if it threw
extern "C" int ddh_cigar_indels_json(const uint8_t *record, int n, char *out, int cap)
{
    std::vector<CigarIndel> indels;
    std::string thrown;
    try { cigarIndels(RawBamView(record, size_t(n)), indels); } catch (const std::string &e) { thrown = e; }
    std::ostringstream os;
    os << "{\"indels\":[";
    for (size_t i = 0; i < indels.size(); i++) os << (i ? "," : "") << "[" << indels[i].refpos << "," << indels[i].len << ",\"" << indels[i].seq << "\"]";
    os << "]";
    if (!thrown.empty()) os << ",\"throw\":\"" << thrown << "\"";
    os << "}";
    return emit(os.str(), out, cap);
}
