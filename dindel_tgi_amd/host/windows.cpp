// windows.cpp — see windows.hpp.  Line references are to the reference's python/makeWindows.py and python/selectCandidates.py.
#include "windows.hpp"
#include <algorithm>
#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <set>
#include <sstream>

namespace dindel {

namespace {

// str.split() of Python: the words between runs of blanks
std::vector<std::string> words(const std::string &line)
{
    std::vector<std::string> w;
    size_t i = 0;
    while (i < line.size()) {
        while (i < line.size() && strchr(" \t\n\r\v\f", line[i])) i++;
        size_t e = i;
        while (e < line.size() && !strchr(" \t\n\r\v\f", line[e])) e++;
        if (e > i) w.push_back(line.substr(i, e - i));
        i = e;
    }
    return w;
}

// int(s) of Python for a decimal literal: an optional sign and digits.  false: Python raises ValueError
bool parseInt(const std::string &s, long &v)
{
    size_t i = (!s.empty() && (s[0] == '-' || s[0] == '+')) ? 1 : 0;
    if (i == s.size()) return false;
    for (size_t k = i; k < s.size(); k++) if (s[k] < '0' || s[k] > '9') return false;
    errno = 0;
    v = strtol(s.c_str(), NULL, 10);
    return errno == 0;
}

long intOrThrow(const std::string &s)
{
    long v = 0;
    if (!parseInt(s, v)) throw std::string("invalid literal for int() with base 10: '").append(s).append("'");
    return v;
}

long floorDiv(long a, long b) { return a / b - ((a % b != 0 && ((a < 0) != (b < 0))) ? 1 : 0); }

// class Variant, python/makeWindows.py:5-31: the reference span of one variant string at refPos
void variantSpan(long refPos, const std::string &s, long &refStart, long &refEnd)
{
    if (s.size() < 2) throw std::string("Unrecognized variant: ").append(s);
    const long length = long(s.size()) - 1;
    refStart = refPos;
    if (s[0] == '-') refEnd = refPos + length - 1;
    else if (s[0] == '+') refEnd = refPos - 1;
    else if (s.size() == 4) refEnd = refPos;
    else throw std::string("Unrecognized variant: ").append(s);
}

const long kHapWidth = 60, kMaxVarPerWindow = 16;        // python/makeWindows.py:34

struct Target {
    std::string name;
    std::map<long, std::vector<std::string> > at;        // position -> its variant strings in input order, repeats included
};

} // namespace

std::vector<long> clusterKeys(const std::vector<long> &positions, long minDist)
{
    std::vector<long> keys(positions.size());
    for (size_t p = 0; p < positions.size(); p++)
        keys[p] = (p > 0 && positions[p] - positions[p - 1] <= minDist) ? keys[p - 1] : positions[p];
    return keys;
}

void makeWindows(const std::vector<std::string> &lines, long minDist, long numWindowsPerFile, std::vector<WindowFile> &files, std::ostream &err,
                 std::ostream *progress)
{
    // python/makeWindows.py:133-163
    std::vector<Target> targets;                         // in order of first appearance
    std::map<std::string, size_t> targetOf;
    long numVar = 0, numread = 0;
    for (size_t l = 0; l < lines.size(); l++) {
        const std::vector<std::string> dat = words(lines[l]);
        if (dat.size() < 2) throw std::string("list index out of range");
        const long pos = intOrThrow(dat[1]);
        numread++;
        if (progress && numread % 10000 == 1) *progress << numread << " lines read\n";
        long chrno = 0;
        if (parseInt(dat[0], chrno) && (chrno > 24 || chrno == 0)) err << "Chromosome number>24. Are you sure this is correct?\n";
        std::map<std::string, size_t>::const_iterator it = targetOf.find(dat[0]);
        if (it == targetOf.end()) {
            it = targetOf.insert(std::make_pair(dat[0], targets.size())).first;
            targets.push_back(Target());
            targets.back().name = dat[0];
        }
        std::vector<std::string> &here = targets[it->second].at[pos];
        for (size_t i = 2; i < dat.size() && dat[i] != "#"; i++) { here.push_back(dat[i]); numVar++; }
    }
    err << "Total variants read: " << numVar << "\n";
    err << "Number of chromosomes: " << targets.size() << "\n";                       // python/makeWindows.py:167-169
    for (size_t t = 0; t < targets.size(); t++) err << "\tchr " << targets[t].name << ": " << targets[t].at.size() << "\n";

    int idx = files.empty() ? 0 : files.back().number;
    for (size_t t = 0; t < targets.size(); t++) {
        const Target &T = targets[t];
        std::vector<long> positions;
        for (std::map<long, std::vector<std::string> >::const_iterator it = T.at.begin(); it != T.at.end(); ++it) positions.push_back(it->first);
        const std::vector<long> keys = clusterKeys(positions, minDist);               // python/makeWindows.py:177-186
        long totVar = 0;
        for (size_t p = 0; p < positions.size(); p++) totVar += long(T.at.find(positions[p])->second.size());
        err << "Chromosome: " << T.name << " Total lines: " << totVar << " at minimum distance " << minDist << "\n";   // :202
        err.flush();

        // write_output_candidates, python/makeWindows.py:34-125: called once per target, so every target starts a file
        long numLineWritten = 10000000, tot = 0, totCand = 0, maxSize = 0, sumSize = 0;
        for (size_t p = 0; p < positions.size();) {
            size_t e = p + 1;
            while (e < positions.size() && keys[e] == keys[p]) e++;
            if (numLineWritten > numWindowsPerFile) {                                 // :48-57
                files.push_back(WindowFile());
                files.back().number = ++idx;
                numLineWritten = 0;
            } else numLineWritten++;
            // the cluster's distinct (position, variant) pairs: by position, then by first appearance (:64 walks a set)
            std::vector<std::pair<long, std::string> > vars;
            long minRef = 2000000000, maxRef = 0;
            for (size_t q = p; q < e; q++) {
                const std::vector<std::string> &here = T.at.find(positions[q])->second;
                std::set<std::string> seen;
                for (size_t k = 0; k < here.size(); k++) {
                    if (!seen.insert(here[k]).second) continue;
                    long refStart = 0, refEnd = 0;
                    variantSpan(positions[q], here[k], refStart, refEnd);
                    vars.push_back(std::make_pair(refStart, here[k]));
                    totCand++;
                    if (refStart < minRef) minRef = refStart;
                    if (refEnd > maxRef) maxRef = refEnd;
                }
            }
            const long leftPos = std::max(0L, minRef - kHapWidth), rightPos = maxRef + kHapWidth;        // :72-75
            const long wsize = rightPos - leftPos;
            if (tot == 0 || wsize > maxSize) maxSize = wsize;
            sumSize += wsize;
            for (size_t vc = 0; vc < vars.size();) {                                  // :89-107
                std::ostringstream line;
                line << T.name << " " << leftPos << " " << rightPos;
                for (long k = 0; k < kMaxVarPerWindow && vc < vars.size(); k++, vc++) line << " " << vars[vc].first << "," << vars[vc].second;
                files.back().lines.push_back(line.str());
            }
            tot++;
            p = e;
        }
        if (tot == 0) throw std::string("max() arg is an empty sequence");            // (:116; no target is without a position)
        err << "Number of candidates: " << totCand << " Number of windows: " << tot << " Maximum window size: " << maxSize
            << " Mean window size: " << floorDiv(sumSize, tot) << "\n";               // :114-117
    }
}

std::vector<std::string> selectCandidates(const std::vector<std::string> &lines, long minCount, long maxCount, std::ostream &err)
{
    std::vector<std::string> out;
    std::set<std::string> visited;
    // the buffer: one position's variants in order of first appearance, with their summed counts
    std::vector<std::pair<std::string, long> > buffer;
    std::string currChr;
    bool haveChr = false;
    long currPos = -1, bufferPos = -1;
    struct Empty {                                                                    // emptyBuffer, python/selectCandidates.py:6-10
        static void run(std::vector<std::string> &out, const std::vector<std::pair<std::string, long> > &buffer, long pos, const std::string &chrom,
                        long minCount, long maxCount)
        {
            for (size_t k = 0; k < buffer.size(); k++) if (buffer[k].second >= minCount && buffer[k].second <= maxCount) {
                std::ostringstream line;
                line << chrom << " " << pos << " " << buffer[k].first << " # " << buffer[k].second;
                out.push_back(line.str());
            }
        }
    };
    for (size_t l = 0; l < lines.size(); l++) {
        if (lines[l].empty() && l + 1 == lines.size()) break;
        const std::vector<std::string> dat = words(lines[l]);
        if (dat.size() < 2) throw std::string("list index out of range");
        const long pos = intOrThrow(dat[1]);
        if (!haveChr || dat[0] != currChr) {                                          // python/selectCandidates.py:35-41
            if (visited.count(dat[0])) throw std::string("Chromosome already processed. Please sort with respect to chromosome first and then position!");
            currChr = dat[0]; haveChr = true;
            visited.insert(dat[0]);
            err << "Analyzing chromosome " << dat[0] << "\n";
            currPos = -1;
        }
        if (pos < currPos) throw std::string("Variants not sorted with respect to position (second column)!");
        size_t y = 2;
        while (y < dat.size() && dat[y] != "#") y++;
        // (dat.index('#') finds a '#' in the first two fields too; such a line has no variants)
        if (dat[0] == "#" || dat[1] == "#") y = 2;
        else if (y == dat.size()) throw std::string("'#' is not in list");
        if (pos > currPos) {                                                          // :51-55
            if (currPos != -1) Empty::run(out, buffer, bufferPos, currChr, minCount, maxCount);
            currPos = pos;
            buffer.clear();
            bufferPos = pos;
        }
        if (pos == currPos)                                                           // :57-61
            for (size_t idx = 0; idx + 2 < y; idx++) {
                if (y + 1 + idx >= dat.size()) throw std::string("list index out of range");
                const long count = intOrThrow(dat[y + 1 + idx]);
                size_t k = 0;
                while (k < buffer.size() && buffer[k].first != dat[2 + idx]) k++;
                if (k == buffer.size()) buffer.push_back(std::make_pair(dat[2 + idx], 0L));
                buffer[k].second += count;
            }
    }
    if (haveChr) Empty::run(out, buffer, bufferPos, currChr, minCount, maxCount);     // :63
    return out;
}

long writeWindows(const WindowOptions &opt, std::ostream &err)
{
    std::ifstream in(opt.inputVarFile.c_str());
    if (!in.is_open()) throw std::string("Cannot open file ").append(opt.inputVarFile);
    std::vector<std::string> lines;
    std::string line;
    while (std::getline(in, line)) lines.push_back(line);
    std::ostringstream silent;
    std::ostream &log = opt.quiet ? static_cast<std::ostream &>(silent) : err;
    if (opt.filter) {
        lines = selectCandidates(lines, opt.minCount, opt.maxCount, log);
        if (!opt.selectedFile.empty()) {
            std::ofstream sel(opt.selectedFile.c_str());
            if (!sel.is_open()) throw std::string("Cannot open file ").append(opt.selectedFile).append(" for writing.");
            for (size_t l = 0; l < lines.size(); l++) sel << lines[l] << "\n";
        }
    }
    std::vector<WindowFile> files;
    makeWindows(lines, opt.minDist, opt.numWindowsPerFile, files, log, opt.quiet ? NULL : &std::cout);
    long written = 0;
    std::ofstream one;
    if (!opt.oneFile.empty()) {
        one.open(opt.oneFile.c_str());
        if (!one.is_open()) throw std::string("Cannot open file ").append(opt.oneFile).append(" for writing.");
    }
    for (size_t f = 0; f < files.size(); f++) {
        std::ofstream numbered;
        if (opt.oneFile.empty()) {
            std::ostringstream name;
            name << opt.windowFilePrefix << "." << files[f].number << ".txt";
            numbered.open(name.str().c_str());
            if (!numbered.is_open()) throw std::string("Cannot open file ").append(name.str()).append(" for writing.");
        }
        std::ostream &out = opt.oneFile.empty() ? static_cast<std::ostream &>(numbered) : one;
        for (size_t l = 0; l < files[f].lines.size(); l++, written++) out << files[f].lines[l] << "\n";
    }
    return written;
}

namespace {
const char *kUsage =
    "usage: dindel_windows -i CANDIDATES (-w PREFIX | --oneFile F) [options]       (the reference's python/makeWindows.py)\n"
    "  -i, --inputVarFile F        input file with candidate variants: `tid pos variant ... # count ...` lines\n"
    "  -w, --windowFilePrefix P    prefix of output files with windows: P.1.txt, P.2.txt, ...\n"
    "  -m, --minDist N             mininum distance between two windows (default 20)\n"
    "  -n, --numWindowsPerFile N   number of windows per file (default 1000)\n"
    "  --oneFile F                 write every window line to F instead of the numbered files\n"
    "  --minCount N, --maxCount M  first keep only the variants seen N ... M times (python/selectCandidates.py; given one, the other\n"
    "                              takes its default, 2 / 10000000); the input must be sorted by target, then position\n"
    "  --selectedFile F            with the filter: write what it kept to F, `tid pos variant # count` lines\n"
    "  --quiet                     no summary on stderr, no progress on stdout\n"
    "  -h, --help                  this text\n";
}

int windowsMain(int argc, char **argv)
{
    WindowOptions opt;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        const char *v = i + 1 < argc ? argv[i + 1] : NULL;
        long n = 0;
        if (a == "-h" || a == "--help") { std::cout << kUsage; return 0; }
        else if (a == "--quiet") opt.quiet = true;
        else if ((a == "-i" || a == "--inputVarFile") && v) { opt.inputVarFile = v; i++; }
        else if ((a == "-w" || a == "--windowFilePrefix") && v) { opt.windowFilePrefix = v; i++; }
        else if (a == "--oneFile" && v) { opt.oneFile = v; i++; }
        else if (a == "--selectedFile" && v) { opt.selectedFile = v; i++; }
        else if ((a == "-m" || a == "--minDist" || a == "-n" || a == "--numWindowsPerFile" || a == "--minCount" || a == "--maxCount") && v) {
            if (!parseInt(v, n)) { std::cerr << "dindel_windows: error: option " << a << ": invalid integer value: '" << v << "'\n"; return 2; }
            if (a == "-m" || a == "--minDist") opt.minDist = n;
            else if (a == "-n" || a == "--numWindowsPerFile") opt.numWindowsPerFile = n;
            else if (a == "--minCount") { opt.minCount = n; opt.filter = true; }
            else { opt.maxCount = n; opt.filter = true; }
            i++;
        } else { std::cerr << "dindel_windows: error: no such option, or no value for it: " << a << "\n"; return 2; }
    }
    if (opt.inputVarFile.empty()) { std::cerr << "Please specify --inputVarFile\n"; return 1; }                       // python/makeWindows.py:220-225
    if (opt.windowFilePrefix.empty() && opt.oneFile.empty()) { std::cerr << "Please specify --windowFilePrefix\n"; return 1; }
    try {
        writeWindows(opt, std::cerr);
    } catch (const std::string &s) {
        std::cerr << "An error occurred!\n" << s << "\n";
        return 1;
    }
    return 0;
}

} // namespace dindel
