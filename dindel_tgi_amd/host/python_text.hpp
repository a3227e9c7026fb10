// python_text.hpp — Python 2's string and file primitives as the restated scripts use them (host/vcf_candidates.cpp, host/pooled_vcf.cpp).
// Defined in host/vcf_candidates.cpp.  Where the script would die, `pyRaise` throws std::string: a NameError's own text, any other
// exception as `Type: text`.
#ifndef DINDEL_PYTHON_TEXT_HPP
#define DINDEL_PYTHON_TEXT_HPP
#include <string>
#include <vector>

namespace dindel {
namespace pytext {

extern const char *const kBlanks;                                   // what str.strip() / str.split() take for blanks: " \t\n\r\v\f"
void pyRaise(const char *type, const std::string &text);            // never returns
std::vector<std::string> words(const std::string &line);            // str.split(): the words between runs of blanks
std::vector<std::string> split(const std::string &s, char c);       // str.split(c): every field, empty ones included
std::string strip(const std::string &s);                            // str.strip()
long pyInt(const std::string &s);                                   // int(s): blanks around, an optional sign, decimal digits; else ValueError
std::string ioError(const std::string &path);                       // the text of an IOError for `path` from errno
// the whole file as bytes; a name whose extension is .gz (os.path.splitext) through zlib, member after member (bgzip's output too)
std::string readBytes(const std::string &path);

} // namespace pytext
} // namespace dindel
#endif
