// pooled_vcf.cpp — see pooled_vcf.hpp.  Line references are to the reference's python/mergeOutputPooled.py and
// python/makeGenotypeLikelihoodFilePooled.py and to their FileUtils.py, Variant.py and Fasta.py.
#include "pooled_vcf.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <sstream>
#include <sys/stat.h>
#include "glf_to_vcf.hpp"
#include "python_text.hpp"

namespace dindel {

using namespace pytext;

namespace {

bool pathExists(const std::string &path) { struct stat st; return stat(path.c_str(), &st) == 0; }      // os.path.exists

std::string rstripOf(const std::string &s, const char *chars)
{
    size_t b = s.size();
    while (b > 0 && strchr(chars, s[b - 1])) b--;
    return s.substr(0, b);
}

std::string lower(std::string s)
{
    for (size_t i = 0; i < s.size(); i++) if (s[i] >= 'A' && s[i] <= 'Z') s[i] = char(s[i] - 'A' + 'a');
    return s;
}

std::string tail(const std::string &s, size_t n) { return s.size() <= n ? s : s.substr(s.size() - n); }   // s[-n:]

long floorDiv(long a, long b) { return a / b - ((a % b != 0 && ((a < 0) != (b < 0))) ? 1 : 0); }

std::string quotedKey(const std::string &key) { return std::string("'").append(key).append("'"); }

// FileUtils.FileWithHeader in read mode, FileUtils.py:38-69, :104-137
class Table {
public:
    Table(const std::string &fname, char joinChar, std::ostream &err) : name(fname), join(joinChar), text(readBytes(fname)), at(0), err(err)
    {
        std::string headerLine;
        if (lower(tail(fname, 3)) == "vcf" || lower(tail(fname, 6)) == "vcf.gz") {                        // FileUtils.py:43-50
            for (;;) {
                if (at >= text.size()) pyRaise("IOError", std::string("no header line in '").append(fname).append("'"));   // (the script spins here)
                const std::string line = rstripOf(rawline(), kBlanks);
                if (line.size() >= 2 && line[0] == '#' && line[1] != '#') { headerLine = line.substr(1); break; }
            }
        } else headerLine = rstripOf(rawline(), kBlanks);                                                 // FileUtils.py:53
        labels = split(headerLine, join);
        for (size_t i = 0; i < labels.size(); i++) column[labels[i]] = i;                                 // a repeated label: the last column wins
    }
    enum Got { END, BAD, ROW };
    // readlineList, FileUtils.py:123-137: BAD is the script's None
    Got readlineList(std::vector<std::string> &cells)
    {
        cells = split(rstripOf(rawline(), kBlanks), join);
        if (cells.size() == 1 && cells[0].empty()) return END;
        if (cells.size() != labels.size()) { wrongNumber(); return BAD; }
        return ROW;
    }
    // readline, FileUtils.py:104-122: false is the script's {}
    bool readline(std::vector<std::string> &cells)
    {
        cells = split(rstripOf(rawline(), " "), join);
        if (cells.size() == 1 && cells[0].empty()) return false;
        if (cells.size() != labels.size()) { wrongNumber(); pyRaise("ZeroDivisionError", "integer division or modulo by zero"); }   // FileUtils.py:116
        return true;
    }
    // dat[key] of a row read by readline
    const std::string &cell(const std::vector<std::string> &cells, const char *key) const
    {
        std::map<std::string, size_t>::const_iterator it = column.find(key);
        if (it == column.end()) pyRaise("KeyError", quotedKey(key));
        return cells[it->second];
    }
    size_t numLabels() const { return labels.size(); }

private:
    // f.readline().rstrip("\n"): the next line without its newline; empty at the end of the file
    std::string rawline()
    {
        if (at >= text.size()) return std::string();
        const size_t e = text.find('\n', at);
        const size_t stop = e == std::string::npos ? text.size() : e;
        const std::string line = text.substr(at, stop - at);
        at = e == std::string::npos ? text.size() : e + 1;
        return line;
    }
    void wrongNumber() { err << "Line in file " << name << " does not have the correct number of labels\n"; }

    std::string name;
    char join;
    std::string text;
    size_t at;
    std::ostream &err;
    std::vector<std::string> labels;
    std::map<std::string, size_t> column;
};

// list.index(label) inside the try of python/mergeOutputPooled.py:251-273
size_t requiredColumn(const std::vector<std::string> &headerLabels, const char *label)
{
    for (size_t i = 0; i < headerLabels.size(); i++) if (headerLabels[i] == label) return i;
    pyRaise("NameError", "GLF files are corrupt. Could not find all required columns.");
    return 0;
}

struct VarStat {                                                      // python/mergeOutputPooled.py:375
    double QUAL, AF;
    long NF, NR, NFS, NRS, DP, NS;
    int HP;
    std::string filter;
};
typedef std::map<long, std::map<std::string, VarStat> > ChromStat;    // pos -> variant -> record; std::map: ascending positions, variants in byte order

void openFasta(const std::string &refFile)                            // Fasta.py:31-32, :13: the two open() calls, in their order
{
    for (const std::string &f : {refFile, refFile + ".fai"}) {
        FILE *t = fopen(f.c_str(), "rb");
        if (!t) pyRaise("IOError", ioError(f));
        fclose(t);
    }
}

// the first word of each line of a list file (python/makeGenotypeLikelihoodFilePooled.py:113-116, :161-165)
std::vector<std::string> firstWords(const std::string &listFile)
{
    std::ifstream f(listFile.c_str());
    if (!f.is_open()) pyRaise("IOError", ioError(listFile));
    std::vector<std::string> v;
    std::string line;
    while (std::getline(f, line)) {
        const std::vector<std::string> w = words(line);
        if (w.empty()) pyRaise("IndexError", "list index out of range");
        v.push_back(w[0]);
    }
    return v;
}

} // namespace

std::vector<long> getPercentiles(const std::map<long, long> &hist, const std::vector<int> &pctiles)
{
    std::map<long, long> cum;                                         // :9-18 (std::map walks its keys in ascending order: `vals`)
    long prevk = 0;
    size_t idx = 0;
    for (std::map<long, long>::const_iterator it = hist.begin(); it != hist.end(); ++it, ++idx) {
        cum[it->first] = it->second;
        if (idx > 0) cum[it->first] += cum[prevk];
        prevk = it->first;
    }
    if (!cum.count(0)) cum[0] = 0;                                    // :20-21
    const long tot = cum[prevk];
    std::vector<long> iles_k(pctiles.size(), 0);
    size_t ilidx = 0;
    for (std::map<long, long>::const_iterator it = hist.begin(); it != hist.end(); ++it)                  // :27-30: one step per distinct depth at most
        if (ilidx < pctiles.size() && double(cum[it->first]) > double(pctiles[ilidx]) / 100.0 * double(tot)) iles_k[ilidx++] = it->first;
    return iles_k;
}

std::string pythonStrFloat(double x)
{
    char buf[64];
    snprintf(buf, sizeof buf, "%.12g", x);
    std::string s = buf;
    if (x != x) return "nan";
    if (s.find('.') == std::string::npos && s.find('e') == std::string::npos && s.find("inf") == std::string::npos) s += ".0";
    return s;
}

void pooledGlfToVcf(const std::vector<std::string> &glfFiles, const PooledVcfOptions &opt, std::ostream &err, std::ostream &out)
{
    const int minDist = 10, dbSNPWindow = 50;
    const long minForwardReverse = 1;
    std::vector<std::string> allFiles, headerLabels;
    for (size_t f = 0; f < glfFiles.size(); f++) {                    // :214-236
        const std::string &gf = glfFiles[f];
        if (!pathExists(gf)) { err << "WARNING: GLF file " << gf << " does not exist.\n"; continue; }
        const std::string text = readBytes(gf);
        if (text.empty()) { err << "WARNING: GLF file " << gf << " is empty.\n"; continue; }
        const std::vector<std::string> d = words(text.substr(0, text.find('\n')));
        if (headerLabels.empty()) { headerLabels = d; allFiles.push_back(gf); }
        else if (d != headerLabels) err << "Inconsistent header in GLF file " << gf << "\n";
        else allFiles.push_back(gf);
    }
    openFasta(opt.refFile);
    IndexedFasta fa(opt.refFile);                                     // :241
    const long numInds = opt.numSamples;
    if (numInds == 0) pyRaise("ZeroDivisionError", "float division by zero");
    const double minFreq = 1.0 / (double(2 * numInds) * 5);           // :247

    const size_t realpos_col = requiredColumn(headerLabels, "realigned_position"), var_col = requiredColumn(headerLabels, "nref_all");   // :251-273
    std::ostringstream tc;
    tc << "tc" << minDist;
    const std::string tcFilter = tc.str();
    const size_t col_num_reads = requiredColumn(headerLabels, "num_reads");
    const size_t col_num_forward_old = requiredColumn(headerLabels, "num_cover_forward"), col_num_reverse_old = requiredColumn(headerLabels, "num_cover_reverse");
    const size_t col_num_forward = requiredColumn(headerLabels, "var_coverage_forward"), col_num_reverse = requiredColumn(headerLabels, "var_coverage_reverse");
    const size_t col_post_prob = requiredColumn(headerLabels, "post_prob_variant"), chr_col = requiredColumn(headerLabels, "tid");
    const size_t idx_col = requiredColumn(headerLabels, "indidx"), ana_col = requiredColumn(headerLabels, "analysis_type");

    std::map<std::string, ChromStat> varStat;
    std::map<std::string, std::map<long, std::vector<std::string> > > pass_filters;
    long nr = 0;
    std::map<long, long> rdhist;
    std::vector<std::string> dat;
    // dat[col]: a header with a tab between two labels has fewer columns than labels
    auto cell = [&](size_t col) -> const std::string & { if (col >= dat.size()) pyRaise("IndexError", "list index out of range"); return dat[col]; };
    for (size_t f = 0; f < allFiles.size(); f++) {                    // :282-379
        const std::string &glffile = allFiles[f];
        Table fglf(glffile, ' ', err);
        out << "Reading " << glffile << "\n";
        bool done = false;
        for (;;) {
            long pos = -1;
            std::string var, chr;
            nr++;
            if (nr % 10000 == 9999) out << "Number of lines read: " << nr + 1 << "\n";
            long num_ind_with_data = 0, tot_coverage = 0, tot_num_forward = 0, tot_num_reverse = 0, tot_num_forward_old = 0, tot_num_reverse_old = 0;
            bool skip = false;
            if (opt.numBamFiles < 1) pyRaise("UnboundLocalError", "local variable 'dat' referenced before assignment");   // (:356 with an empty range at :304)
            for (long fidx = 0; fidx < opt.numBamFiles; fidx++) {
                const Table::Got got = fglf.readlineList(dat);
                if (got == Table::END) { done = true; break; }                                            // :313-315
                if (got == Table::BAD) pyRaise("TypeError", "'NoneType' object has no attribute '__getitem__'");   // :316 on the None of FileUtils.py:135
                if (cell(realpos_col) == "NA") { skip = true; break; }
                if (cell(ana_col) != "singlevariant") { skip = true; break; }
                if (cell(idx_col) != "NA" && pyInt(cell(idx_col)) >= opt.numBamFiles) pyRaise("NameError", "Error. Is the number of BAM files correctly specified?");
                if (pos == -1) { pos = pyInt(cell(realpos_col)); var = cell(var_col); chr = cell(chr_col); }
                else if (pyInt(cell(realpos_col)) != pos) pyRaise("NameError", "Inconsistent glf files! Is the number of BAM files correctly specified?");
                if (pyInt(cell(idx_col)) != fidx) err << "Error reading this variant: " << chr << " " << pos << " " << var << " in " << glffile << "\n";
                tot_num_forward_old += pyInt(cell(col_num_forward_old));
                tot_num_reverse_old += pyInt(cell(col_num_reverse_old));
                if (fidx == 0) {                                      // only recorded for the first pool
                    tot_num_forward = pyInt(cell(col_num_forward));
                    tot_num_reverse = pyInt(cell(col_num_reverse));
                }
                const long numreads = pyInt(cell(col_num_reads));
                if (numreads > 0) num_ind_with_data++;
                tot_coverage += numreads;
            }
            if (skip) continue;
            if (done) break;
            const double prob = pythonFloat(cell(col_post_prob));      // of the group's last line, :356-357
            size_t freq_col = headerLabels.size();
            for (size_t i = 0; i < headerLabels.size() && freq_col == headerLabels.size(); i++) if (headerLabels[i] == "est_freq") freq_col = i;
            if (freq_col == headerLabels.size()) pyRaise("ValueError", "'est_freq' is not in list");
            const double freq = pythonFloat(cell(freq_col));
            rdhist[tot_coverage]++;
            if (prob > 0.20) {
                if (!fa.has(chr)) { out << "KeyError:  " << chr << "\n"; pyRaise("NameError", "KeyError"); }    // Fasta.py:38-40
                VarStat v;
                v.HP = homopolymerLength(fa.get(chr, pos + 1 - 25, 50), 25);
                v.QUAL = prob; v.NF = tot_num_forward; v.NR = tot_num_reverse; v.NFS = tot_num_forward_old; v.NRS = tot_num_reverse_old;
                v.DP = tot_coverage; v.NS = num_ind_with_data; v.AF = freq;
                varStat[chr][pos][var] = v;
            }
        }
    }

    const std::vector<long> coverageRange = getPercentiles(rdhist, std::vector<int>({1, 99}));           // :384
    const double fqp = 1.0 - pow(10.0, -double(opt.filterQual) / 10.0);
    std::ostringstream fq, hp;
    fq << "q" << opt.filterQual;
    hp << "hp" << opt.maxHPLen;
    for (std::map<std::string, ChromStat>::iterator c = varStat.begin(); c != varStat.end(); ++c)         // :389-425
        for (ChromStat::iterator p = c->second.begin(); p != c->second.end(); ++p)
            for (std::map<std::string, VarStat>::iterator v = p->second.begin(); v != p->second.end(); ++v) {
                const VarStat &var = v->second;
                std::vector<std::string> filters;
                if (var.QUAL < fqp) filters.push_back(fq.str());
                if ((var.NF < minForwardReverse || var.NR < minForwardReverse) && opt.filterFR) filters.push_back("fr0");
                if (var.DP < coverageRange[0] || var.DP > coverageRange[1]) filters.push_back("ocr");
                if (var.NS < floorDiv(numInds, 2)) filters.push_back("s50");
                if (var.HP > opt.maxHPLen) filters.push_back(hp.str());
                if (var.AF < minFreq) filters.push_back("mf");
                if (filters.empty()) pass_filters[c->first][p->first].push_back(v->first);
                std::string joined;
                for (size_t i = 0; i < filters.size(); i++) joined.append(i ? ";" : "").append(filters[i]);
                v->second.filter = joined;
            }

    std::vector<std::string> chromosomes;                             // :429-433
    for (int c = 1; c < 23; c++) chromosomes.push_back(std::to_string(c));
    chromosomes.push_back("X");
    chromosomes.push_back("Y");
    const size_t named = chromosomes.size();
    for (std::map<std::string, ChromStat>::const_iterator c = varStat.begin(); c != varStat.end(); ++c) {   // the others: ascending byte order (see the header)
        bool known = false;
        for (size_t i = 0; i < named && !known; i++) known = chromosomes[i] == c->first;
        if (!known) chromosomes.push_back(c->first);
    }

    out << "Writing VCF\n";
    std::ofstream fv(opt.outputFile.c_str(), std::ios::binary);
    if (!fv.is_open()) pyRaise("IOError", ioError(opt.outputFile));
    fv << "##fileformat=VCFv4.0\n" << "##source=Dindel\n" << "##reference=" << opt.refFile << "\n"         // :439-460
       << "##INFO=<ID=NS,Number=1,Type=Integer,Description=\"Number of samples with data\">\n"
       << "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Total number of reads in haplotype window\">\n"
       << "##INFO=<ID=HP,Number=1,Type=Integer,Description=\"Reference homopolymer tract length\">\n"
       << "##INFO=<ID=NFS,Number=1,Type=Integer,Description=\"Number of reads covering non-ref variant site on forward strand\">\n"
       << "##INFO=<ID=NRS,Number=1,Type=Integer,Description=\"Number of reads covering non-ref variant site on reverse strand\">\n"
       << "##INFO=<ID=NF,Number=1,Type=Integer,Description=\"Number of reads covering non-ref variant on forward strand\">\n"
       << "##INFO=<ID=NR,Number=1,Type=Integer,Description=\"Number of reads covering non-ref variant on reverse strand\">\n"
       << "##INFO=<ID=AF,Number=-1,Type=Float,Description=\"Allele frequency\">\n"
       << "##INFO=<ID=DB,Number=0,Type=Flag,Description=\"dbSNP membership build 129 - type match and indel sequence length match within " << dbSNPWindow << " bp\">\n"
       << "##FILTER=<ID=q" << opt.filterQual << ",Description=\"Quality below " << opt.filterQual << "\">\n"
       << "##FILTER=<ID=s50,Description=\"Less than 50% of samples have data\">\n"
       << "##FILTER=<ID=tc" << minDist << ",Description=\"Indel site was closer than " << minDist << " base pairs from another site with higher posterior probability\">\n"
       << "##FILTER=<ID=hp" << opt.maxHPLen << ",Description=\"Reference homopolymer length was longer than " << opt.maxHPLen << "\">\n";
    if (opt.filterFR) fv << "##FILTER=<ID=fr0,Description=\"Non-ref allele is not covered by at least one read on both strands\">\n";
    fv << "##FILTER=<ID=ocr,Description=\"Number of reads in haplotype window outside coverage range " << coverageRange[0] << " " << coverageRange[1] << "\">\n"
       << "##FILTER=<ID=mf,Description=\"Too low non-ref allele frequency\">\n"
       << "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";

    std::string altseq;                                               // (the script's altseq outlives an iteration: a `ref`-type string writes the one before)
    bool haveAltseq = false;
    for (size_t ci = 0; ci < chromosomes.size(); ci++) {              // :463-574
        const std::string &chr = chromosomes[ci];
        if (!pass_filters.count(chr)) continue;                       // no PASS variant: no line at all, :464-465
        ChromStat &stat = varStat[chr];
        std::vector<long> positions;
        for (std::map<long, std::vector<std::string> >::const_iterator p = pass_filters[chr].begin(); p != pass_filters[chr].end(); ++p) positions.push_back(p->first);
        std::vector<long> newPosition = positions;
        for (bool done = false; !done;) {                             // :471-477
            done = true;
            for (size_t p = 1; p < positions.size(); p++)
                if (newPosition[p] != newPosition[p - 1] && newPosition[p] - positions[p - 1] <= minDist) { newPosition[p] = newPosition[p - 1]; done = false; }
        }
        std::map<long, std::vector<long> > newSites;                  // merged site -> its positions, ascending (:479-491)
        for (size_t p = 0; p < newPosition.size(); p++) newSites[newPosition[p]].push_back(positions[p]);
        out << "New number of sites: " << newSites.size() << "\n" << "Number of sites filtered: " << long(pass_filters[chr].size()) - long(newSites.size()) << "\n";
        for (std::map<long, std::vector<long> >::const_iterator s = newSites.begin(); s != newSites.end(); ++s) {   // :499-531
            const std::vector<long> &old = s->second;
            size_t best = 0;
            double bestProb = 0.0;
            for (size_t o = 0; o < old.size(); o++) {
                double max_prob = -1.0;
                for (std::map<std::string, VarStat>::const_iterator v = stat[old[o]].begin(); v != stat[old[o]].end(); ++v) if (v->second.QUAL > max_prob) max_prob = v->second.QUAL;
                if (o == 0 || max_prob > bestProb) { best = o; bestProb = max_prob; }                     // the first of the largest: the lowest position on a tie
            }
            for (size_t o = 0; o < old.size(); o++) {
                if (o == best) continue;
                for (std::map<std::string, VarStat>::iterator v = stat[old[o]].begin(); v != stat[old[o]].end(); ++v)
                    if (!v->second.filter.empty()) v->second.filter.append(";").append(tcFilter);         // (:529: a PASS variant stays PASS)
            }
        }
        out << "Number of indel sites: " << newSites.size() << "\n";
        for (ChromStat::const_iterator p = stat.begin(); p != stat.end(); ++p)                            // :537-574
            for (std::map<std::string, VarStat>::const_iterator v = p->second.begin(); v != p->second.end(); ++v) {
                const long pos = p->first;
                const std::string &var = v->first;
                const VarStat &st = v->second;
                long indel_report_pos = pos;
                const long qual = -long(10.0 * log10(std::max(1.0 - st.QUAL, 1e-10)));
                std::ostringstream info;
                info << "AF=" << pythonStrFloat(st.AF) << ";NS=" << st.NS << ";DP=" << st.DP << ";HP=" << st.HP << ";NF=" << st.NF << ";NR=" << st.NR << ";NFS=" << st.NFS
                     << ";NRS=" << st.NRS;
                if (var.empty()) pyRaise("IndexError", "string index out of range");                        // Variant.py:7
                const VariantString vnref(var);
                const int max_del_len = vnref.type == VariantString::DEL ? vnref.length : 0;
                std::string refseq = fa.get(chr, indel_report_pos, 1 + max_del_len);
                if (vnref.type == VariantString::DEL) {
                    if (refseq.empty()) pyRaise("IndexError", "string index out of range");
                    altseq = refseq.substr(0, 1) + (refseq.size() > size_t(1 + vnref.length) ? refseq.substr(size_t(1 + vnref.length)) : std::string());
                    haveAltseq = true;
                } else if (vnref.type == VariantString::INS) {
                    if (refseq.empty()) pyRaise("IndexError", "string index out of range");
                    altseq = refseq.substr(0, 1) + vnref.seq + refseq.substr(1);
                    haveAltseq = true;
                } else if (vnref.type == VariantString::SNP) {
                    indel_report_pos += 1;
                    if (refseq.size() < 2) pyRaise("IndexError", "string index out of range");              // :563: refseq has one letter
                    refseq = refseq.substr(1, 1);
                    altseq = vnref.seq.substr(0, 1);
                    haveAltseq = true;
                }
                if (!haveAltseq) pyRaise("UnboundLocalError", "local variable 'altseq' referenced before assignment");
                fv << chr << "\t" << indel_report_pos << "\t.\t" << refseq << "\t" << altseq << "\t" << qual << "\t" << (st.filter.empty() ? std::string("PASS") : st.filter)
                   << "\t" << info.str() << "\n";
            }
    }
    fv.close();
    if (!fv) pyRaise("IOError", std::string("error writing '").append(opt.outputFile).append("'"));
}

void processPooledGLFFiles(const std::string &glfFilesFile, const PooledVcfOptions &opt, std::ostream &err, std::ostream &out)
{
    std::ifstream f(glfFilesFile.c_str());                            // :209-213
    if (!f.is_open()) pyRaise("IOError", ioError(glfFilesFile));
    std::vector<std::string> files;
    std::string line;
    while (std::getline(f, line)) {
        const std::vector<std::string> w = words(line);
        files.insert(files.end(), w.begin(), w.end());
    }
    pooledGlfToVcf(files, opt, err, out);
}

Variant4 variant4AnyLength(const std::string &ref, const std::string &alt)
{
    if (ref.size() != alt.size()) return variant4(ref, alt);
    Variant4 v;                                                       // Variant.py:37-62
    int nm = 0;
    char refnuc = 0, altnuc = 0;
    for (size_t idx = 0; idx < ref.size(); idx++)
        if (ref[idx] != alt[idx]) { nm++; v.offset = int(idx); refnuc = ref[idx]; altnuc = alt[idx]; }
    if (nm == 0) pyRaise("AttributeError", "Variant4 instance has no attribute 'offset'");                  // type "ref": the offset is never set and getCalls reads it
    if (nm > 1) pyRaise("NameError", "MultiSNP");
    v.type = "snp";
    v.seq = std::string(1, altnuc);
    v.str = std::string(1, refnuc) + "=>" + v.seq;
    return v;
}

namespace {

typedef std::map<std::string, std::map<long, std::map<std::string, bool> > > Calls;

// getCalls, python/makeGenotypeLikelihoodFilePooled.py:10-46
void getCalls(const std::string &callFile, Calls &calls, std::ostream &err, std::ostream &out)
{
    Table vcf(callFile, '\t', err);
    long numcalls = 0;
    std::vector<std::string> dat;
    while (vcf.readline(dat)) {
        const std::string &filter = vcf.cell(dat, "FILTER");
        if (!(filter == "PASS" || (filter == "q20" && pythonFloat(vcf.cell(dat, "QUAL")) >= 10))) continue;
        const std::string chrom = vcf.cell(dat, "CHROM");
        const long pos = pyInt(vcf.cell(dat, "POS"));
        const std::string ref = vcf.cell(dat, "REF"), alt = vcf.cell(dat, "ALT");
        if (alt.find(',') != std::string::npos) pyRaise("NameError", "Cannot deal with these entries");
        const Variant4 var = variant4AnyLength(ref, alt);
        const long newpos = pos + var.offset - 1;                     // zero-based
        if (calls[chrom][newpos].count(var.str)) pyRaise("NameError", "Multiple same variants?");
        calls[chrom][newpos][var.str] = true;
        numcalls++;
    }
    out << "Number of calls imported: " << numcalls << "\n";
}

// loadGLFFiles behind its list, python/makeGenotypeLikelihoodFilePooled.py:118-141
std::vector<std::string> orderGLFFiles(const std::vector<std::string> &glffiles, std::ostream &err, std::ostream &out)
{
    std::map<long, std::string> fp_to_fname;
    std::vector<std::string> dat;
    for (size_t f = 0; f < glffiles.size(); f++) {
        if (!pathExists(glffiles[f])) { err << "File " << glffiles[f] << " does not exist\n"; continue; }
        Table fg(glffiles[f], ' ', err);
        for (;;) {
            if (!fg.readline(dat)) pyRaise("KeyError", "'realigned_position'");                             // :127 on the {} of the file's end
            const std::string &rp = fg.cell(dat, "realigned_position");
            if (rp == "NA") continue;
            const long firstpos = pyInt(rp);
            if (fp_to_fname.count(firstpos)) pyRaise("NameError", "Huh?");
            fp_to_fname[firstpos] = glffiles[f];
            break;
        }
    }
    std::vector<std::string> ordered;
    for (std::map<long, std::string>::const_iterator it = fp_to_fname.begin(); it != fp_to_fname.end(); ++it) {
        out << "pos: " << it->first << " glffile: " << it->second << "\n";
        ordered.push_back(it->second);
    }
    return ordered;
}

typedef std::vector<std::vector<std::string> > Group;

// emptyBuffer, python/makeGenotypeLikelihoodFilePooled.py:49-107; true is "a-ok"
bool emptyBuffer(const std::string &index, std::map<std::string, Group> &buffer, const Table &fg, const Calls &calls, std::ostream &fout,
                 const std::vector<std::string> &bamfiles, std::ostream &err)
{
    std::map<std::string, Group>::iterator b = buffer.find(index);
    if (b == buffer.end()) pyRaise("KeyError", quotedKey(index));       // (a file without a data line: buffer['-1'])
    const Group &glfs = b->second;
    const std::vector<std::string> &first = glfs[0];
    if (fg.cell(first, "nref_all") == "NA") { buffer.erase(b); return false; }                            // na-error
    const std::string varstring = fg.cell(first, "tid") + " " + fg.cell(first, "realigned_position") + " " + fg.cell(first, "nref_all");
    {                                                                 // :67-71: KeyError alone is caught; int() of the position is inside the try and is not
        Calls::const_iterator c = calls.find(fg.cell(first, "tid"));
        bool called = c != calls.end();
        const long pos = called ? pyInt(fg.cell(first, "realigned_position")) : 0;
        if (called) {
            std::map<long, std::map<std::string, bool> >::const_iterator p = c->second.find(pos);
            called = p != c->second.end() && p->second.count(fg.cell(first, "nref_all"));
        }
        if (!called) { buffer.erase(b); return false; }               // notcalled
    }
    if (glfs.size() != bamfiles.size()) {                             // :74-77
        err << "Skipping index " << index << "\n";
        buffer.erase(b);
        return false;
    }
    std::string output;
    for (size_t g = 0; g < glfs.size(); g++) {                        // :84-99
        const std::vector<std::string> &dat = glfs[g];
        if (fg.cell(dat, "tid") + " " + fg.cell(dat, "realigned_position") + " " + fg.cell(dat, "nref_all") != varstring) return false;   // (left in the buffer)
        long idx = pyInt(fg.cell(dat, "indidx"));
        const std::vector<std::string> liks = split(fg.cell(dat, "glf"), ';');
        std::map<std::string, std::string> gen_to_lik;
        for (size_t l = 0; l < liks.size(); l++) {
            const std::vector<std::string> ld = split(liks[l], ':');
            if (ld.size() < 2) pyRaise("IndexError", "list index out of range");
            gen_to_lik[ld[0]] = ld[1];
        }
        const long position = pyInt(fg.cell(dat, "realigned_position"));
        for (const char *g2 : {"0/0", "0/1", "1/1"}) if (!gen_to_lik.count(g2)) pyRaise("KeyError", quotedKey(g2));
        if (idx < 0) idx += long(bamfiles.size());                    // (a negative index counts from the end of a Python list)
        if (idx < 0 || idx >= long(bamfiles.size())) pyRaise("IndexError", "list index out of range");
        std::ostringstream os;
        os << fg.cell(dat, "tid") << " " << position << " " << fg.cell(dat, "nref_all") << " " << gen_to_lik["0/0"] << " " << gen_to_lik["0/1"] << " " << gen_to_lik["1/1"]
           << " " << bamfiles[size_t(idx)] << "\n";
        output += os.str();
    }
    fout << output;
    buffer.erase(b);
    return true;
}

} // namespace

namespace {
typedef std::function<std::vector<std::string>()> NameList;

// makeGLF, python/makeGenotypeLikelihoodFilePooled.py:146-213: the calls, the .glf.txt files, the BAM names, the output file, in this order
void callsToGlf(const NameList &glfFiles, const std::string &callFile, const std::string &outputFile, const NameList &bamNames, std::ostream &err, std::ostream &out)
{
    Calls calls;
    out << "Reading VCF file\n";
    getCalls(callFile, calls, err, out);
    out << "done\n";
    const std::vector<std::string> glffiles = orderGLFFiles(glfFiles(), err, out);
    const std::vector<std::string> bamfiles = bamNames();
    long numwritten = 0;
    std::ofstream fout(outputFile.c_str(), std::ios::binary);         // :173
    if (!fout.is_open()) pyRaise("IOError", ioError(outputFile));
    std::vector<std::string> dat;
    for (size_t f = 0; f < glffiles.size(); f++) {                    // :175-209
        out << "Checking " << glffiles[f] << "\n";
        Table fg(glffiles[f], ' ', err);
        std::map<std::string, Group> buffer;
        std::string curr_index = "-1";
        while (fg.readline(dat)) {
            const std::string newindex = fg.cell(dat, "index") + "." + fg.cell(dat, "realigned_position") + "." + fg.cell(dat, "nref_all");
            buffer[newindex].push_back(dat);
            if (newindex != curr_index) {
                if (curr_index != "-1" && emptyBuffer(curr_index, buffer, fg, calls, fout, bamfiles, err)) numwritten++;
                curr_index = newindex;
            }
        }
        if (emptyBuffer(curr_index, buffer, fg, calls, fout, bamfiles, err)) numwritten++;
        out << "Number written: " << numwritten << "\n";
    }
    fout.close();
    if (!fout) pyRaise("IOError", std::string("error writing '").append(outputFile).append("'"));
}
} // namespace

void pooledCallsToGlf(const std::vector<std::string> &glfFiles, const std::string &callFile, const std::string &outputFile,
                      const std::vector<std::string> &bamNames, std::ostream &err, std::ostream &out)
{
    callsToGlf([&]() { return glfFiles; }, callFile, outputFile, [&]() { return bamNames; }, err, out);
}

void makeGLF(const std::string &inputGLFFiles, const std::string &outputFile, const std::string &callFile, const std::string &bamfilesFile,
             std::ostream &err, std::ostream &out)
{
    callsToGlf([&]() { return firstWords(inputGLFFiles); }, callFile, outputFile, [&]() { return firstWords(bamfilesFile); }, err, out);
}

} // namespace dindel
