// pooled_capi.cpp — the extern "C" hook of host/pooled_em.cpp for the pytest suite (ctypes), in the pattern of windows_capi.cpp.  Not part
// of the drop-in boundary.
#include <cstring>
#include "pooled_em_text.hpp"

using namespace dindel;

// One window written as text (pooled_em_text.hpp) -> its pooled .glf.txt lines; the EM slots run on the CPU.  Returns the length, the
// negative length needed when `cap` is too small, or -1 with the message in `out`.
extern "C" int ddh_pooled_window_lines(const char *text, const char *program, double a0, double priorSNP, double priorIndel, char *out, int cap)
{
    std::string s;
    int rc = 0;
    try { s = pooledLinesOfText(text ? text : "", program ? program : "", a0, priorSNP, priorIndel); }
    catch (std::string &e) { s = e; rc = -1; }
    catch (std::exception &e) { s = e.what(); rc = -1; }
    if (int(s.size()) + 1 > cap) return rc ? -1 : -int(s.size()) - 1;
    memcpy(out, s.c_str(), s.size() + 1);
    return rc ? -1 : int(s.size());
}
