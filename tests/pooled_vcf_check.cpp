// pooled_vcf_check.cpp — host/pooled_vcf.cpp on its own, for a build under AddressSanitizer and UBSan (tests/test_pooled_vcf_cpu.py compiles it
// with host/pooled_vcf.cpp, host/vcf_candidates.cpp and host/glf_to_vcf.cpp and runs it as a program).  Both conversions run over generated
// .glf.txt files and over malformed ones; what they throw is caught and counted, and the program says what it saw.
//
//   pooled_vcf_check DIR        (an empty directory to write into)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../dindel_tgi_amd/host/pooled_vcf.hpp"

using namespace dindel;

namespace {

uint64_t state = 88172645463325252ull;
uint32_t rnd(uint32_t n) { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return uint32_t(state % n); }

const char *const kHeader =
    "msg index analysis_type tid lpos rpos center_position realigned_position was_candidate_in_window ref_all nref_all num_reads post_prob_variant qual est_freq "
    "logZ hapfreqs indidx msq numOffAll num_indel num_cover_forward num_cover_reverse num_unmapped_realigned var_coverage_forward var_coverage_reverse nBQT nmmBQT "
    "mLogBQ nMMLeft nMMRight glf\n";

std::string line(int index, const std::string &analysis, const std::string &tid, const std::string &pos, const std::string &var, int reads, const std::string &prob,
                 const std::string &freq, const std::string &indidx, const std::string &glf)
{
    std::ostringstream os;
    os << "ok " << index << " " << analysis << " " << tid << " 40 160 100 " << pos << " 1 NA " << var << " " << reads << " " << prob << " NA " << freq
       << " -123.5 NA " << indidx << " NA NA NA " << rnd(9) << " " << rnd(9) << " NA " << rnd(5) << " " << rnd(5) << " NA NA NA NA NA " << glf << "\n";
    return os.str();
}

void put(const std::string &path, const std::string &text) { std::ofstream f(path.c_str(), std::ios::binary); f << text; }

std::string slurp(const std::string &path) { std::ifstream f(path.c_str(), std::ios::binary); std::ostringstream os; os << f.rdbuf(); return os.str(); }

std::string generated(int sites, int pools, const std::vector<std::string> &tids, int chromLen)
{
    static const char *const vars[] = {"-A", "-AC", "+G", "+TTT", "-ACGTACGT", "+C"};
    static const char *const probs[] = {"0.99999", "0.9995", "0.9", "0.5", "0.1", "1", "0.999"};
    std::string text = kHeader;
    int pos = 30;
    size_t t = 0;
    for (int s = 0; s < sites; s++) {
        pos += 1 + int(rnd(14));
        if (pos > chromLen - 40) { pos = 30; t = (t + 1) % tids.size(); }
        const std::string var = vars[rnd(6)], prob = probs[rnd(7)];
        if (rnd(17) == 0) text += line(s, "NA", tids[t], "NA", "NA", 0, "NA", "NA", "NA", "NA");             // a skipped window
        for (int b = 0; b < pools; b++)
            text += line(s, "singlevariant", tids[t], std::to_string(pos), var, int(rnd(40)), prob, "0.25", std::to_string(b), "0/0:-10.5;0/1:-2.25;1/1:-30");
        if (rnd(5) == 0) text += line(s, "dip.map", tids[t], std::to_string(pos), var, 20, "NA", "0.5", "0", "*/*:-40.5;*/" + var + ":-2.5");
    }
    return text;
}

int thrown = 0;

template <class F> void attempt(const char *what, F f)
{
    try { f(); } catch (const std::string &s) { thrown++; if (getenv("POOLED_VCF_CHECK_VERBOSE")) std::cout << "  " << what << ": " << s << "\n"; }
}

} // namespace

int main(int argc, char **argv)
{
    if (argc != 2) { std::cerr << "usage: pooled_vcf_check DIR\n"; return 2; }
    const std::string d = std::string(argv[1]) + "/";
    const int chromLen = 3000;
    const std::vector<std::string> tids = {"1", "2", "X", "chrUn"};
    {                                                                  // the FASTA and its index
        std::string fa, fai;
        for (size_t t = 0; t < tids.size(); t++) {
            fa += ">" + tids[t] + "\n";
            std::ostringstream os;
            os << tids[t] << "\t" << chromLen << "\t" << fa.size() << "\t60\t61\n";
            fai += os.str();
            for (int i = 0; i < chromLen; i++) { fa += "ACGT"[rnd(7) < 3 ? 0 : rnd(4)]; if (i % 60 == 59) fa += "\n"; }
        }
        put(d + "ref.fa", fa);
        put(d + "ref.fa.fai", fai);
    }
    std::ostringstream err, out;
    PooledVcfOptions opt;
    opt.refFile = d + "ref.fa"; opt.outputFile = d + "out.vcf"; opt.numSamples = 4; opt.numBamFiles = 3; opt.filterFR = true;

    // generated input: both conversions, the second on what the first wrote
    const std::string good = generated(300, 3, tids, chromLen);
    put(d + "good.glf.txt", good);
    pooledGlfToVcf(std::vector<std::string>(1, d + "good.glf.txt"), opt, err, out);
    const std::string vcf = slurp(d + "out.vcf");
    size_t records = 0;
    for (size_t i = 0; i + 1 < vcf.size(); i++) records += vcf[i] == '\n' && vcf[i + 1] != '#';
    std::vector<std::string> bams = {"a.bam", "b.bam", "c.bam"};
    pooledCallsToGlf(std::vector<std::string>(1, d + "good.glf.txt"), d + "out.vcf", d + "out.glf", bams, err, out);
    const std::string glf = slurp(d + "out.glf");
    size_t glfLines = 0;
    for (size_t i = 0; i < glf.size(); i++) glfLines += glf[i] == '\n';
    std::cout << "generated: " << records << " VCF records, " << glfLines << " likelihood lines\n";
    if (records == 0 || glfLines == 0 || glfLines % 3 != 0) { std::cerr << "nothing was called\n"; return 1; }
    put(d + "list.txt", d + "good.glf.txt " + d + "none.glf.txt\n\n" + d + "good.glf.txt\n");
    put(d + "bams.txt", "a.bam x\nb.bam\nc.bam\n");
    processPooledGLFFiles(d + "list.txt", opt, err, out);
    put(d + "glflist.txt", d + "good.glf.txt\n");
    makeGLF(d + "glflist.txt", d + "out2.glf", d + "out.vcf", d + "bams.txt", err, out);
    if (slurp(d + "out2.glf") != glf) { std::cerr << "makeGLF and pooledCallsToGlf differ\n"; return 1; }

    // malformed input: every prefix length of a small file in steps, lines cut, fields dropped, garbage
    const std::string small = generated(12, 3, tids, chromLen);
    int cuts = 0;
    for (size_t n = 0; n <= small.size(); n += 97, cuts++) {
        put(d + "cut.glf.txt", small.substr(0, n));
        attempt("cut", [&]() { pooledGlfToVcf(std::vector<std::string>(1, d + "cut.glf.txt"), opt, err, out); });
        attempt("cut", [&]() { pooledCallsToGlf(std::vector<std::string>(1, d + "cut.glf.txt"), d + "out.vcf", d + "cut.glf", bams, err, out); });
    }
    for (int k = 0; k < 80; k++) {                                     // one byte of the small file changed
        std::string t = small;
        t[size_t(rnd(uint32_t(t.size())))] = " \n\t:;,=>*+-0/Nx"[rnd(15)];
        put(d + "mut.glf.txt", t);
        attempt("mutated", [&]() { pooledGlfToVcf(std::vector<std::string>(1, d + "mut.glf.txt"), opt, err, out); });
        attempt("mutated", [&]() { pooledCallsToGlf(std::vector<std::string>(1, d + "mut.glf.txt"), d + "out.vcf", d + "mut.glf", bams, err, out); });
    }
    for (int k = 0; k < 80; k++) {                                     // one byte of the VCF changed
        std::string t = vcf;
        t[size_t(rnd(uint32_t(t.size())))] = " \n\t:;,=>*+-0/Nx#"[rnd(16)];
        put(d + "mut.vcf", t);
        attempt("mutated calls", [&]() { pooledCallsToGlf(std::vector<std::string>(1, d + "good.glf.txt"), d + "mut.vcf", d + "mut.glf", bams, err, out); });
    }
    put(d + "snp.glf.txt", std::string(kHeader) + line(1, "singlevariant", "1", "100", "A=>C", 20, "0.99999", "0.25", "0", "x") + line(2, "singlevariant", "1", "200", "-A", 30, "0.1", "0.25", "0", "x"));
    PooledVcfOptions one = opt;
    one.numBamFiles = 1; one.filterFR = false;
    attempt("snp", [&]() { pooledGlfToVcf(std::vector<std::string>(1, d + "snp.glf.txt"), one, err, out); });
    put(d + "garbage.glf.txt", std::string("\x01\x02 \xff\n\n\x00 a b", 11));
    attempt("garbage", [&]() { pooledGlfToVcf(std::vector<std::string>(1, d + "garbage.glf.txt"), opt, err, out); });
    attempt("garbage", [&]() { pooledCallsToGlf(std::vector<std::string>(1, d + "garbage.glf.txt"), d + "out.vcf", d + "g.glf", bams, err, out); });
    attempt("no calls file", [&]() { pooledCallsToGlf(std::vector<std::string>(1, d + "good.glf.txt"), d + "none.vcf", d + "g.glf", bams, err, out); });
    attempt("no fasta", [&]() { PooledVcfOptions o = opt; o.refFile = d + "none.fa"; pooledGlfToVcf(std::vector<std::string>(1, d + "good.glf.txt"), o, err, out); });
    attempt("numSamples 0", [&]() { PooledVcfOptions o = opt; o.numSamples = 0; pooledGlfToVcf(std::vector<std::string>(1, d + "good.glf.txt"), o, err, out); });
    attempt("numBamFiles 0", [&]() { PooledVcfOptions o = opt; o.numBamFiles = 0; pooledGlfToVcf(std::vector<std::string>(1, d + "good.glf.txt"), o, err, out); });
    for (const char *pair : {"A A", "AC AT", "ACG TCA", "AC A", "A AC", " A", "A ", " "}) {
        const std::string p = pair, ref = p.substr(0, p.find(' ')), alt = p.substr(p.find(' ') + 1);
        attempt("variant4", [&]() { variant4AnyLength(ref, alt); });
    }
    std::map<long, long> hist;
    for (int k = 0; k < 50; k++) { hist[long(rnd(30)) - 3] = long(rnd(100)); getPercentiles(hist, std::vector<int>({1, 5, 50, 99})); }
    std::cout << "malformed: " << cuts << " cuts, " << thrown << " conversions died as the scripts do\nok\n";
    return thrown > 0 ? 0 : 1;
}
