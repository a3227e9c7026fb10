// vcf_candidates.cpp — see vcf_candidates.hpp.  Line references are to the reference's python/convertVCFToDindel.py and its
// python/utils/VCFFile.py, python/utils/Variant.py and python/utils/Fasta.py.
#include "vcf_candidates.hpp"
#include "python_text.hpp"
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <set>
#include <sstream>
#include <vector>
#include <zlib.h>

namespace dindel {

namespace pytext {

// where the script dies: a NameError's own text, any other exception as `Type: text`
void pyRaise(const char *type, const std::string &text)
{
    if (!strcmp(type, "NameError")) throw text;
    throw std::string(type).append(": ").append(text);
}

const char *const kBlanks = " \t\n\r\v\f";

// str.split() of Python: the words between runs of blanks
std::vector<std::string> words(const std::string &line)
{
    std::vector<std::string> w;
    size_t i = 0;
    while (i < line.size()) {
        while (i < line.size() && strchr(kBlanks, line[i])) i++;
        size_t e = i;
        while (e < line.size() && !strchr(kBlanks, line[e])) e++;
        if (e > i) w.push_back(line.substr(i, e - i));
        i = e;
    }
    return w;
}

// str.split(c) of Python: every field, empty ones included
std::vector<std::string> split(const std::string &s, char c)
{
    std::vector<std::string> f;
    size_t i = 0;
    for (;;) {
        const size_t e = s.find(c, i);
        if (e == std::string::npos) { f.push_back(s.substr(i)); return f; }
        f.push_back(s.substr(i, e - i));
        i = e + 1;
    }
}

std::string strip(const std::string &s)
{
    size_t a = 0, b = s.size();
    while (a < b && strchr(kBlanks, s[a])) a++;
    while (b > a && strchr(kBlanks, s[b - 1])) b--;
    return s.substr(a, b - a);
}

// int(s) of Python 2 for a string: blanks around, an optional sign, decimal digits
long pyInt(const std::string &s)
{
    const std::string t = strip(s);
    size_t i = (!t.empty() && (t[0] == '-' || t[0] == '+')) ? 1 : 0;
    bool ok = i < t.size();
    for (size_t k = i; k < t.size() && ok; k++) ok = t[k] >= '0' && t[k] <= '9';
    if (!ok) pyRaise("ValueError", std::string("invalid literal for int() with base 10: '").append(s).append("'"));
    errno = 0;
    const long v = strtol(t.c_str(), NULL, 10);
    if (errno != 0) pyRaise("OverflowError", std::string("integer too large for this tool: '").append(s).append("'"));
    return v;
}

} // namespace pytext
using namespace pytext;

double pythonFloat(const std::string &s)
{
    const std::string t = strip(s);
    bool ok = !t.empty();
    for (size_t k = 0; k < t.size() && ok; k++) ok = t[k] != 'x' && t[k] != 'X' && t[k] != '(' && !strchr(kBlanks, t[k]);
    char *end = NULL;
    const double v = ok ? strtod(t.c_str(), &end) : 0.0;
    if (!ok || end == t.c_str() || *end != '\0') pyRaise("ValueError", std::string("could not convert string to float: ").append(s));
    return v;
}

namespace {

long floorDiv(long a, long b) { return a / b - ((a % b != 0 && ((a < 0) != (b < 0))) ? 1 : 0); }
long floorMod(long a, long b) { return a - floorDiv(a, b) * b; }

std::string upperNoSpaces(const std::string &s)               // string.upper(s.replace(' ', ''))
{
    std::string u;
    for (size_t i = 0; i < s.size(); i++) if (s[i] != ' ') u += (s[i] >= 'a' && s[i] <= 'z') ? char(s[i] - 'a' + 'A') : s[i];
    return u;
}

} // namespace

namespace pytext {
std::string ioError(const std::string &path) { return std::string("[Errno ") + std::to_string(errno) + "] " + strerror(errno) + ": '" + path + "'"; }

// the whole file as bytes; a name whose extension is .gz (python/utils/VCFFile.py:95-98) through zlib, member after member
std::string readBytes(const std::string &path)
{
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) pyRaise("IOError", ioError(path));
    std::string raw;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) raw.append(buf, n);
    fclose(f);
    // os.path.splitext: from the last dot of the last component, the dots it starts with aside
    size_t first = path.rfind('/') == std::string::npos ? 0 : path.rfind('/') + 1;
    while (first < path.size() && path[first] == '.') first++;
    const size_t dot = path.rfind('.');
    const bool gz = dot != std::string::npos && dot >= first && path.compare(dot, std::string::npos, ".gz") == 0;
    if (!gz) return raw;
    std::string text;
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, 15 + 16) != Z_OK) pyRaise("IOError", "zlib: inflateInit2 failed");
    z.next_in = reinterpret_cast<Bytef *>(const_cast<char *>(raw.data()));
    z.avail_in = uInt(raw.size());
    if (raw.size() > size_t(0x7fffffff)) { inflateEnd(&z); pyRaise("IOError", "compressed VCF larger than 2 GiB"); }
    bool ended = raw.empty();                                 // (no member at all: an empty file)
    while (z.avail_in > 0) {
        z.next_out = reinterpret_cast<Bytef *>(buf);
        z.avail_out = uInt(sizeof buf);
        const int rc = inflate(&z, Z_NO_FLUSH);
        text.append(buf, sizeof buf - z.avail_out);
        ended = rc == Z_STREAM_END;
        if (ended) {                             // the next member, if any (zero padding behind the last one is allowed, as in gzip.py)
            while (z.avail_in > 0 && *z.next_in == 0) { z.next_in++; z.avail_in--; }
            if (z.avail_in > 0 && inflateReset(&z) != Z_OK) { inflateEnd(&z); pyRaise("IOError", "zlib: inflateReset failed"); }
        } else if (rc != Z_OK) {
            inflateEnd(&z);
            pyRaise("IOError", rc == Z_BUF_ERROR ? "Compressed file ended before the end-of-stream marker was reached" : "Not a gzipped file");
        }
    }
    inflateEnd(&z);
    if (!ended) pyRaise("IOError", "Compressed file ended before the end-of-stream marker was reached");
    return text;
}
} // namespace pytext

namespace {

// class FastaIndex and Fasta.get, python/utils/Fasta.py:11-51
class ScriptFasta {
public:
    explicit ScriptFasta(const std::string &fname) : fa(fopen(fname.c_str(), "rb"))
    {
        if (!fa) pyRaise("IOError", ioError(fname));
        std::ifstream fai((fname + ".fai").c_str());
        if (!fai.is_open()) { const std::string e = ioError(fname + ".fai"); fclose(fa); fa = NULL; pyRaise("IOError", e); }
        std::string line;
        try {
            while (std::getline(fai, line)) {
                const std::vector<std::string> dat = words(line);
                if (dat.size() != 5) continue;
                Target t;
                t.len = pyInt(dat[1]); t.offset = pyInt(dat[2]); t.blen = pyInt(dat[3]); t.llen = pyInt(dat[4]);
                ft[dat[0]] = t;
            }
        } catch (...) { fclose(fa); fa = NULL; throw; }
    }
    ~ScriptFasta() { if (fa) fclose(fa); }
    std::string get(const std::string &tid, long pos1based, size_t len, std::ostream &out)
    {
        const long pos = pos1based - 1;
        std::map<std::string, Target>::const_iterator it = ft.find(tid);
        if (it == ft.end()) {
            out << "KeyError:  " << tid << "\n";
            pyRaise("NameError", "KeyError");
        }
        const Target &idx = it->second;
        if (idx.blen == 0) pyRaise("ZeroDivisionError", "integer division or modulo by zero");
        const long fpos = idx.offset + floorDiv(pos, idx.blen) * idx.llen + floorMod(pos, idx.blen);
        if (fpos < 0) pyRaise("IOError", "[Errno 22] Invalid argument");
        std::string seq;
        if (fseek(fa, fpos, SEEK_SET) != 0) pyRaise("IOError", "[Errno 22] Invalid argument");
        for (size_t numread = 0; numread < len;) {
            const int c = getc(fa);
            if (c == EOF) break;                              // every further read gives '' and counts: the letters come out short
            if (c != '\n') { seq += char(c); numread++; }
        }
        return seq;
    }
private:
    struct Target { long len, offset, blen, llen; };
    FILE *fa;
    std::map<std::string, Target> ft;
    ScriptFasta(const ScriptFasta &); ScriptFasta &operator=(const ScriptFasta &);
};

// VCFFile in read mode, python/utils/VCFFile.py:75-352: what the conversion needs of it, and every way it dies
class VcfReader {
public:
    VcfReader(const std::string &fname, std::ostream &err) : text(readBytes(fname)), at(0), version(0), err(err)
    {
        bool infoFound = false;
        for (;;) {
            const std::string line = readline();
            if (line.compare(0, 2, "##") == 0) {
                if (line.find("fileformat") != std::string::npos) {                                       // :103-112
                    if (line.find("VCF") == std::string::npos && line.find("vcf") == std::string::npos) pyRaise("NameError", "Cannot determine VCF version");
                    if (line.find("v3") != std::string::npos) version = 3;
                    else if (line.find("v4") != std::string::npos || line.find("VCF4") != std::string::npos) version = 4;
                    else pyRaise("NameError", "Cannot determine VCF version");
                }
                if (line.compare(0, 7, "##INFO=") == 0) { description(line, 7, info, true); infoFound = true; }   // :115-169
                else if (line.compare(0, 9, "##FILTER=") == 0) description(line, 9, filter, false);              // :170-206
                else if (line.compare(0, 9, "##FORMAT=") == 0) description(line, 9, format, true);               // :210-257
            } else {                                                                                      // :267: line[0] == '#' and line[1] == 'C'
                if (line.empty()) pyRaise("IndexError", "string index out of range");
                if (line[0] != '#') continue;
                if (line.size() < 2) pyRaise("IndexError", "string index out of range");
                if (line[1] != 'C') continue;
                if (!infoFound) err << "WARNING: did not detect INFO fields!\n";
                std::string headerLine;
                for (size_t i = 0; i < line.size(); i++) if (line[i] != '#') headerLine += line[i];
                labels = words(headerLine);
                for (size_t i = 0; i < labels.size(); i++) column[labels[i]] = i;
                break;
            }
        }
        static const char *const mainLabels[] = {"CHROM", "POS", "ID", "REF", "ALT", "QUAL"};
        for (size_t k = 0; k < 6; k++)                                                                    // :280-282
            if (!column.count(mainLabels[k])) pyRaise("NameError", std::string("Could not find column ").append(mainLabels[k]).append(" in header of VCF file!"));
        minLen = 0;                                                                                       // :284
        for (std::map<std::string, size_t>::const_iterator it = column.begin(); it != column.end(); ++it) if (it->second > minLen) minLen = it->second;
    }

    struct Record { std::string chrom, pos, ref, alt, qual; };
    // readline / parseline, :287-352.  false: the {} that ends the file's conversion
    bool next(Record &r)
    {
        const std::string line = readline();
        if (line.empty()) return false;
        const std::vector<std::string> col = split(line, '\t');
        if (col.size() < minLen) {
            err << "Cannot parse this line:\n" << line << "\n";
            return false;
        }
        // :298-302 read the main columns, then every other labelled column; :307 the INFO column, :324 the FILTER column
        for (std::map<std::string, size_t>::const_iterator it = column.begin(); it != column.end(); ++it)
            if (it->first != "INFO" && it->first != "FILTER" && it->second >= col.size()) pyRaise("IndexError", "list index out of range");
        for (const char *lab : {"INFO", "FILTER"}) {
            if (!column.count(lab)) pyRaise("KeyError", std::string("'").append(lab).append("'"));
            if (column[lab] >= col.size()) pyRaise("IndexError", "list index out of range");
        }
        if (version == 0) pyRaise("AttributeError", "VCFFile instance has no attribute 'version'");         // :333
        r.chrom = col[column["CHROM"]]; r.pos = col[column["POS"]]; r.ref = col[column["REF"]]; r.alt = col[column["ALT"]]; r.qual = col[column["QUAL"]];
        return true;
    }

private:
    // f.readline().rstrip('\n'): the next line without its newline(s); empty at the end of the file
    std::string readline()
    {
        if (at >= text.size()) return std::string();
        size_t e = text.find('\n', at);
        const size_t stop = e == std::string::npos ? text.size() : e;
        std::string line = text.substr(at, stop - at);
        at = e == std::string::npos ? text.size() : e + 1;
        return line;
    }
    // fields[i] of a version-4 description must be KEY=value
    std::string keyed(const std::vector<std::string> &fields, size_t i, const char *key, const std::string &line)
    {
        if (i >= fields.size()) pyRaise("IndexError", "list index out of range");
        const std::vector<std::string> pair = split(fields[i], '=');
        if (upperNoSpaces(pair[0]) != key) pyRaise("NameError", std::string("Could not find ").append(key).append(" in: ").append(line));
        if (pair.size() < 2) pyRaise("IndexError", "list index out of range");
        return pair[1];
    }
    // one ##INFO= / ##FILTER= / ##FORMAT= line; `full`: number and type are part of it
    void description(const std::string &line, size_t skip, std::set<std::string> &ids, bool full)
    {
        const std::string sstr = line.substr(skip);
        size_t quotes = 0;
        for (size_t i = 0; i < sstr.size(); i++) quotes += sstr[i] == '"';
        if (quotes != 2) pyRaise("NameError", std::string("Incomplete description: ").append(line));
        if (version == 0) pyRaise("AttributeError", "VCFFile instance has no attribute 'version'");
        if (version < 4) {
            const std::vector<std::string> fields2 = split(split(sstr, '"')[0], ',');
            const std::string id = fields2[0];
            if (full) {
                if (fields2.size() < 2) pyRaise("IndexError", "list index out of range");
                if (fields2[1] != ".") pyInt(fields2[1]);
                if (fields2.size() < 3) pyRaise("IndexError", "list index out of range");
            }
            if (ids.count(id)) pyRaise("NameError", std::string("VCF file already has info-id ").append(id));
            ids.insert(id);
        } else {
            if (sstr[0] != '<' || sstr[sstr.size() - 1] != '>') pyRaise("NameError", "Incorrect description");
            const std::vector<std::string> fields = split(sstr.substr(1, sstr.size() - 2), ',');
            ids.insert(keyed(fields, 0, "ID", line));
            if (full) { keyed(fields, 1, "NUMBER", line); keyed(fields, 2, "TYPE", line); keyed(fields, 3, "DESCRIPTION", line); }
            else keyed(fields, 1, "DESCRIPTION", line);
        }
    }

    std::string text;
    size_t at;
    int version;                                             // 0: no fileformat line yet
    std::ostream &err;
    std::set<std::string> info, filter, format;
    std::vector<std::string> labels;
    std::map<std::string, size_t> column;                    // lab_to_col
    size_t minLen;
};

} // namespace

Variant4 variant4(const std::string &ref, const std::string &alt)
{
    Variant4 v;
    const bool ins = ref.size() < alt.size();
    v.type = ins ? "ins" : "del";
    const std::string &longer = ins ? alt : ref, &shorter = ins ? ref : alt;              // _alt, _ref of python/utils/Variant.py:67-76
    const size_t numrb = shorter.size();
    size_t leftMatch = 0, rightMatch = 0;
    while (leftMatch < numrb && shorter[leftMatch] == longer[leftMatch]) leftMatch++;
    while (rightMatch < numrb && shorter[numrb - 1 - rightMatch] == longer[longer.size() - 1 - rightMatch]) rightMatch++;
    if (leftMatch == 0 || leftMatch + rightMatch < numrb) pyRaise("NameError", "Don't think this is a proper VCF4 insertion");
    size_t leftEnd = 1;
    if (numrb - leftEnd > rightMatch) leftEnd = leftMatch;
    const size_t rightStart = numrb - leftEnd;                                            // (0: the slice runs to the end, which is the same)
    v.seq = longer.substr(leftEnd, longer.size() - rightStart - leftEnd);
    v.offset = int(leftEnd);
    v.str = (ins ? "+" : "-") + v.seq;
    return v;
}

long convertVcfToCandidates(const VcfConvertOptions &opt, std::ostream &err, std::ostream &out)
{
    std::ofstream fo(opt.outputFile.c_str());
    if (!fo.is_open()) pyRaise("IOError", ioError(opt.outputFile));
    ScriptFasta fa(opt.refFile);
    long written = 0;
    const std::vector<std::string> vcffiles = split(opt.inputFiles, ',');
    for (size_t f = 0; f < vcffiles.size(); f++) {
        VcfReader vcf(vcffiles[f], err);
        VcfReader::Record dat;
        while (vcf.next(dat)) {
            const long pos = pyInt(dat.pos);
            const std::string rseq = fa.get(dat.chrom, pos, dat.ref.size(), out);
            if (rseq != dat.ref) err << "REFSEQ inconsistency\n";
            if (!(dat.qual == "." || pythonFloat(dat.qual) >= opt.minQual)) continue;
            const std::vector<std::string> altseq = split(dat.alt, ',');
            for (size_t a = 0; a < altseq.size(); a++) {
                if (altseq[a] == "<DEL>" || altseq[a].size() == dat.ref.size()) continue;
                const Variant4 var = variant4(dat.ref, altseq[a]);
                const long at = pos + var.offset - 1;
                if (opt.haveRegion && !(dat.chrom == opt.tid && at >= opt.start && at < opt.end)) continue;
                fo << dat.chrom << " " << at << " " << var.str << "\n";
                written++;
            }
        }
    }
    fo.close();
    if (!fo) pyRaise("IOError", std::string("error writing '").append(opt.outputFile).append("'"));
    return written;
}

} // namespace dindel
