// windows_check.cpp — a stand-alone check of host/windows.cpp for a sanitizer build (no Python, no GPU):
//   g++ -std=c++11 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/windows_check.cpp dindel_tgi_amd/host/windows.cpp
//       -o windows_check && ./windows_check
// The window maker and the filter over the inputs of the committed fixtures (the lines of tests/golden/make_windows.json, restated
// here: the program reads no file) and over seeded random inputs — malformed lines, every variant shape, clusters of more than 16, tiny
// files — with the invariants checked that hold for any input: the closed-form clustering against the fixed-point loop, every token
// inside its line's bounds, no more than 16 tokens per line, file numbers rising by one, and the filter's counts within its bounds.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <sstream>
#include <string>
#include <vector>
#include "../dindel_tgi_amd/host/windows.hpp"

using namespace dindel;

namespace {

int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

unsigned long long state = 88172645463325252ULL;
unsigned rnd(unsigned n) { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return unsigned(state % n); }

std::vector<long> fixedPointLoop(const std::vector<long> &positions, long minDist)       // the script's loop, as written
{
    std::vector<long> n(positions);
    bool done = false;
    while (!done) {
        done = true;
        for (size_t p = 1; p < positions.size(); p++)
            if (n[p] != n[p - 1] && n[p] - positions[p - 1] <= minDist) { n[p] = n[p - 1]; done = false; }
    }
    return n;
}

std::vector<std::string> split(const std::string &s)
{
    std::vector<std::string> w;
    std::istringstream is(s);
    std::string x;
    while (is >> x) w.push_back(x);
    return w;
}

// runs both entry points over `lines`; returns the number of window lines, or -1 if either threw
long run(const std::vector<std::string> &lines, long minDist, long perFile, bool filter, long minCount, long maxCount)
{
    std::ostringstream err;
    std::vector<std::string> in(lines);
    std::vector<WindowFile> files;
    try {
        if (filter) {
            in = selectCandidates(in, minCount, maxCount, err);
            for (size_t l = 0; l < in.size(); l++) {
                const std::vector<std::string> w = split(in[l]);
                CHECK(w.size() == 5 && w[3] == "#");
                if (w.size() == 5) { const long c = atol(w[4].c_str()); CHECK(c >= minCount && c <= maxCount); }
            }
        }
        makeWindows(in, minDist, perFile, files, err);
    } catch (const std::string &) { return -1; }
    long n = 0;
    for (size_t f = 0; f < files.size(); f++) {
        CHECK(files[f].number == int(f) + 1);
        for (size_t l = 0; l < files[f].lines.size(); l++, n++) {
            const std::vector<std::string> w = split(files[f].lines[l]);
            CHECK(w.size() >= 4 && w.size() <= 3 + 16);
            const long left = atol(w[1].c_str()), right = atol(w[2].c_str());
            CHECK(left >= 0);
            for (size_t k = 3; k < w.size(); k++) {
                const size_t comma = w[k].find(',');
                CHECK(comma != std::string::npos);
                const long pos = atol(w[k].c_str());
                CHECK(left <= pos - 60 || left == 0);
                CHECK(right >= pos + 59);
            }
        }
    }
    return n;
}

std::string randomVariant()
{
    static const char *const shapes[] = {"-", "+", "A=>C", "ACG", "", "x", "-ACGTACGTAC", "+G", "-T", "+CA", "-GG", "G=>T", "#"};
    if (rnd(150) == 0) return shapes[rnd(sizeof(shapes) / sizeof(*shapes))];
    std::string s(1, "+-"[rnd(2)]);
    for (unsigned k = 1 + rnd(5); k > 0; k--) s += "ACGT"[rnd(4)];
    return s;
}

} // namespace

int main()
{
    // the fixtures' inputs
    const char *const fixtureLines[][8] = {
        {"chr1 1000 -AC # 3", "chr1 1020 +G # 2", "chr1 1041 -T # 1", "chr1 1062 -TT # 1", NULL},
        {"chr1 500 -A # 1", "chr1 515 +CA # 1", "chr1 530 -GG # 1", "chr1 545 +T # 1", "chr1 600 -C # 1", NULL},
        {"chr2 100 -A # 1", "chr2 300 -C # 1", "chr1 200 +GT # 4", "chr2 310 +A # 1", "25 77 -A # 1", "0 90 +C # 1", NULL},
        {"chr1 30 -ACG # 2", "chr1 200 -A # 1", NULL},
        {"chr1 5 +AC # 2", NULL},
        {"chr1 0 +A # 2", NULL},
        {"chr1 700 A=>C -AC # 1 1", "chr1 900 G=>T # 1", NULL},
        {"chr1 100 -AC -AC +G # 1 1 1", "chr1 100 +G -T # 1 1", "chr1 105 -AC # 1", NULL},
        {"chr1 100 -A # 1", "chr1 101 -C # 1", "chr1 101 +G # 1", "chr1 103 -T # 1", NULL},
        {"chr1 900 -A", "chr1 100 +CC", "chr1 940 -G", "chr1 145 -T", "chr1 191 -AA", NULL},
        {"chr1 100 -A # 1", "chr1 200 ACG # 1", NULL},
        {"chr1 100 - # 1", NULL},
        {"chr1 100 -A +C # 1 2", "chr1 100 -A # 1", "chr1 150 -G # 1", "chr1 160 +T -CC # 5 1", "chr1 160 -CC # 1", "chr1 400 -A # 7", NULL},
        {"chr1 100 -A # 2", "chr1 200 -C # 2", "chr2 50 +G # 3", "chr2 60 -T # 1", NULL},
        {"chr1 100 -A # 2", "chr2 50 +G # 3", "chr1 300 -C # 2", NULL},
        {"chr1 100 -A # 2", "chr1 90 +G # 3", NULL},
    };
    for (size_t c = 0; c < sizeof(fixtureLines) / sizeof(*fixtureLines); c++) {
        std::vector<std::string> lines;
        for (size_t k = 0; fixtureLines[c][k]; k++) lines.push_back(fixtureLines[c][k]);
        for (long minDist = 0; minDist <= 45; minDist += 15)
            for (long perFile = 1; perFile <= 3; perFile += 2) {
                run(lines, minDist, perFile, false, 0, 0);
                run(lines, minDist, perFile, true, 1, 4);
                run(lines, minDist, perFile, true, 2, 10000000);
            }
    }
    // clusters of 16, 17, 32 and 33 variants, as the generator of the fixtures makes them
    const int sizes[] = {16, 17, 32, 33};
    for (size_t s = 0; s < 4; s++) {
        std::string line = "chr1 1000";
        for (int k = 0; k < sizes[s]; k++) { line += " -"; for (int j = 0; j < 4; j++) line += "ACGT"[(k >> (2 * j)) & 3]; }
        const long n = run(std::vector<std::string>(1, line), 20, 1000, false, 0, 0);
        CHECK(n == (sizes[s] + 15) / 16);
    }
    // the clustering
    for (int it = 0; it < 2000; it++) {
        std::vector<long> positions;
        long at = long(rnd(500)) - 20;
        for (unsigned n = rnd(41); n > 0; n--) { at += 1 + long(rnd(45)); positions.push_back(at); }
        const long minDist = long(rnd(36)) - 5;
        CHECK(clusterKeys(positions, minDist) == fixedPointLoop(positions, minDist));
    }
    // random inputs, well-formed and not
    long threw = 0, wrote = 0;
    for (int it = 0; it < 3000; it++) {
        std::vector<std::string> lines;
        const bool sorted = rnd(3) != 0;
        long pos = 0;
        for (unsigned n = rnd(30); n > 0; n--) {
            std::ostringstream line;
            pos = sorted ? pos + long(rnd(40)) : long(rnd(3000)) - 5;
            line << (sorted ? (2 * n < 15 ? "chrB" : "chrA") : (rnd(12) == 0 ? "chrB" : "chrA")) << " ";
            if (rnd(400) == 0) line << "x"; else line << pos;
            const unsigned k = rnd(20) == 0 ? 40 : rnd(4);
            for (unsigned v = 0; v < k; v++) line << " " << randomVariant();
            if (rnd(300)) { line << " #"; for (unsigned v = 0; v < k + (rnd(300) == 0 ? 0 : 1) - 1 + (rnd(9) == 0); v++) line << " " << rnd(5); }
            if (rnd(400) == 0) line.str("");
            lines.push_back(line.str());
        }
        const long n = run(lines, long(rnd(31)), 1 + long(rnd(4)), rnd(2) != 0, long(rnd(3)), 2 + long(rnd(6)));
        if (n < 0) threw++; else wrote += n;
    }
    std::printf("windows_check: %ld random inputs threw, %ld window lines written, %d failures\n", threw, wrote, failures);
    CHECK(threw > 100 && wrote > 1000);
    return failures ? 1 : 0;
}
