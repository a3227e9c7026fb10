// candidates.cpp — see candidates.hpp.  The alignment of every candidate (SeqAn in the reference) is the device's; this file restates what
// the reference does around it, quirks included.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <set>
#include <sstream>
#include "align_haplotypes.hpp"
#include "candidates.hpp"

namespace dindel {

// reference GetCandidates.cpp:64-101
void cigarIndels(const RawBamView &rec, std::vector<CigarIndel> &out)
{
    uint32_t refPos = uint32_t(rec.pos());
    int32_t readAt = 0;
    for (uint32_t k = 0; k < rec.nCigar(); k++) {
        const uint32_t word = rec.cigar(k);
        const int op = int(word & 15u);
        const int32_t len = int32_t(word >> 4);
        switch (op) {
            case BAM_CINS: {
                std::string letters;
                for (int32_t x = 0; x < len; x++) letters += rec.base(readAt + x);
                out.push_back(CigarIndel(refPos, len, letters));
                readAt += len;
                break;
            }
            case BAM_CDEL:
                out.push_back(CigarIndel(refPos, -len, std::string(size_t(len), 'D')));
                refPos += uint32_t(len);
                break;
            case BAM_CMATCH: readAt += len; refPos += uint32_t(len); break;
            case BAM_CREF_SKIP: refPos += uint32_t(len); break;
            case BAM_CSOFT_CLIP: readAt += len; break;
            case BAM_CHARD_CLIP: break;
            default: throw std::string("I don't know how to smoke this CIGAR");
        }
    }
}

void addCandidate(CandidateTable &t, const CigarIndel &id)
{
    CandidateTable::iterator it = t.find(int(id.refpos));
    if (it == t.end()) t[int(id.refpos)][id] = 1; else (it->second)[id]++;
}

void alignmentEvents(const int16_t *refPos, int hapLen, int refLen, std::vector<dd_align_events> &out)
{
    out.clear();
    int consumed = 0;                 // reference bases in front of the columns written so far
    bool pairedSeen = false;
    int runAt = -1;                   // index in `out` of the insertion the previous base belongs to
    for (int b = 0; b < hapLen; b++) {
        const int v = refPos[b];
        const bool facesGap = DD_ALIGN_IS_GAP(v);
        const int left = facesGap ? DD_ALIGN_GAP_REFS(v) : v;
        if (left > consumed) {        // deleted reference bases in front of this base
            if (pairedSeen) { const dd_align_events e = {DD_ALIGN_EVENT_DEL, int16_t(consumed), int16_t(left - consumed), int16_t(b)}; out.push_back(e); }
            consumed = left;
            runAt = -1;
        }
        if (!facesGap) { pairedSeen = true; consumed = left + 1; runAt = -1; continue; }
        if (left == 0 || left >= refLen) { runAt = -1; continue; }             // LO / RO
        if (runAt >= 0) out[size_t(runAt)].len++;
        else { const dd_align_events e = {DD_ALIGN_EVENT_INS, int16_t(left), 1, int16_t(b)}; runAt = int(out.size()); out.push_back(e); }
    }
}

std::string fetchReference(IndexedFasta &fa, const std::string &tid, long begin1, long end1)
{
    const long len = fa.length(tid);
    if (len < 0) return std::string();
    if (begin1 < 1) begin1 = 1;
    if (end1 > len) end1 = len;
    if (begin1 > end1) return std::string();
    std::string s = fa.get(tid, begin1, int(end1 - begin1 + 1));
    for (size_t i = 0; i < s.size(); i++) s[i] = char(toupper((unsigned char)s[i]));
    return s;
}

namespace {

const int kAlignWindow = 100;          // GetCandidates.hpp:55

struct Job { size_t cand; int startRef; std::string ref, hap; };
typedef std::vector<std::pair<int, std::string> > Found;      // (position, "+SEQ" | "-SEQ") of one candidate, in key order

void foundFromEvents(const Job &j, const dd_align_events *ev, int n, Found &found)
{
    std::map<int, std::string> byKey;           // hap.indels is a map keyed by the reference offset: a later event at a key replaces an earlier one
    for (int k = 0; k < n; k++) {
        const bool ins = ev[k].kind == DD_ALIGN_EVENT_INS;
        const std::string &from = ins ? j.hap : j.ref;
        const int at = ins ? ev[k].hap : ev[k].ref;
        if (at < 0 || ev[k].len < 0 || size_t(at) + size_t(ev[k].len) > from.size()) throw std::string("indel event outside its sequence");
        std::string s(1, ins ? '+' : '-');
        for (int x = 0; x < ev[k].len; x++) s += dnaLetter(from[size_t(at + x)]);
        byKey[ev[k].ref] = s;
    }
    found.clear();
    for (std::map<int, std::string>::const_iterator it = byKey.begin(); it != byKey.end(); ++it) found.push_back(std::make_pair(j.startRef + it->first, it->second));
}

void foundFromSlice(const Job &j, const int16_t *slice, bool convert, Found &found)
{
    if (!convert) {
        std::vector<dd_align_events> ev;
        alignmentEvents(slice, int(j.hap.size()), int(j.ref.size()), ev);
        foundFromEvents(j, ev.data(), int(ev.size()), found);
        return;
    }
    Haplotype h(j.hap);
    convertHaplotypeAlignment(j.ref, h, std::vector<int>(slice, slice + j.hap.size()));
    found.clear();
    for (std::map<int, AlignedVariant>::const_iterator it = h.indels.begin(); it != h.indels.end(); ++it)
        if (it->second.isIndel()) found.push_back(std::make_pair(j.startRef + it->first, it->second.getString()));
}

struct Packed {
    std::vector<int32_t> refOff, hapOff, pairRef;
    std::string refAll, hapAll;
    dd_align_batch b;
    Packed(const std::vector<Job> &jobs, const std::vector<size_t> &which) : refOff(1, 0), hapOff(1, 0)
    {
        for (size_t k = 0; k < which.size(); k++) {
            const Job &j = jobs[which[k]];
            refAll += j.ref; refOff.push_back(int32_t(refAll.size()));
            hapAll += j.hap; hapOff.push_back(int32_t(hapAll.size()));
            pairRef.push_back(int32_t(k));
        }
        b.n_refs = int32_t(which.size()); b.ref_off = refOff.data(); b.ref_seq = refAll.data();
        b.n_pairs = int32_t(which.size()); b.pair_ref = pairRef.data(); b.hap_off = hapOff.data(); b.hap_seq = hapAll.data();
    }
};

bool aligned(const Job &j, int status, const CandidateOptions &opt, CandidateStats &stats)
{
    if (status == DD_ALIGN_OK) return true;
    stats.dropped++;
    if (status == DD_ALIGN_TOO_LONG) stats.tooLong++;
    if (!opt.quiet)
        std::cerr << "Cannot align variant: " << (status == DD_ALIGN_TOO_LONG ? "sequence longer than 4094 bases" : "empty sequence") << " (reference "
                  << j.ref.size() << ", haplotype " << j.hap.size() << " bases at " << j.startRef << ")" << std::endl;
    return false;
}

// slices of the pairs `which` through the hook or dd_align_haplotypes, then the host conversion (convert) or the host event walk
void runSlices(const std::vector<Job> &jobs, const std::vector<size_t> &which, bool convert, const CandidateOptions &opt, CandidateStats &stats,
               std::vector<Found> &results)
{
    if (which.empty()) return;
    Packed p(jobs, which);
    std::vector<int32_t> score(which.size()), status(which.size());
    std::vector<int16_t> refPos(p.hapAll.size() ? p.hapAll.size() : 1);
    if (opt.hook) opt.hook(opt.hookData, &p.b, status.data(), refPos.data());
    else {
        dd_align_result r = { score.data(), status.data(), refPos.data() };
        if (dd_align_haplotypes(&p.b, &r, opt.device) != DD_SUCCESS) throw std::string("dd_align_haplotypes: ") + dd_last_error();
    }
    for (size_t k = 0; k < which.size(); k++) {
        const Job &j = jobs[which[k]];
        if (aligned(j, status[k], opt, stats)) foundFromSlice(j, refPos.data() + p.hapOff[k], convert, results[j.cand]);
    }
}

void runBatch(const std::vector<Job> &jobs, const std::vector<size_t> &which, const CandidateOptions &opt, CandidateStats &stats,
              std::vector<Found> &results)
{
    if (which.empty()) return;
    stats.batches++;
    if (opt.hook || opt.hostConvert) { runSlices(jobs, which, opt.hostConvert, opt, stats, results); return; }
    Packed p(jobs, which);
    const size_t cap = size_t(opt.eventsCap);
    std::vector<int32_t> score(which.size()), status(which.size()), nEvents(which.size());
    std::vector<dd_align_events> events(which.size() * cap);
    dd_align_result r = { score.data(), status.data(), NULL };
    if (dd_align_haplotypes_events(&p.b, &r, nEvents.data(), events.data(), opt.eventsCap, opt.device) != DD_SUCCESS)
        throw std::string("dd_align_haplotypes_events: ") + dd_last_error();
    std::vector<size_t> again;                    // more events than the cap holds: redone from the slice
    for (size_t k = 0; k < which.size(); k++) {
        const Job &j = jobs[which[k]];
        if (!aligned(j, status[k], opt, stats)) continue;
        if (size_t(nEvents[k]) > cap) { again.push_back(which[k]); continue; }
        foundFromEvents(j, events.data() + k * cap, nEvents[k], results[j.cand]);
    }
    stats.overflowed += long(again.size());
    runSlices(jobs, again, true, opt, stats, results);
}

std::vector<std::string> splitWords(const std::string &line)
{
    std::vector<std::string> w;
    std::istringstream in(line);
    std::string s;
    while (in >> s) w.push_back(s);
    return w;
}

} // namespace

// reference GetCandidates.cpp:197-258 with :103-195 inside
void outputIndels(const std::string &tid, const CandidateTable &table, std::ostream &out, IndexedFasta &fa, const CandidateOptions &opt,
                  CandidateStats &stats)
{
    std::vector<int> counts;
    std::vector<Job> jobs;
    std::vector<size_t> narrow, wide;
    size_t nCand = 0;
    for (CandidateTable::const_iterator it = table.begin(); it != table.end(); ++it) {
        for (std::map<CigarIndel, int>::const_iterator i2 = it->second.begin(); i2 != it->second.end(); ++i2, ++nCand) {
            const CigarIndel &id = i2->first;
            counts.push_back(i2->second);
            stats.candidates++;
            int width = kAlignWindow;
            if (std::abs(id.len) > width / 3) width = std::abs(id.len) * 3;
            const int start = int(id.refpos) - width, end = int(id.refpos) + width;
            Job j;
            j.cand = nCand; j.startRef = start;
            j.ref = fetchReference(fa, tid, long(start) + 1, long(end) + 1);
            if (j.ref.empty()) {
                std::cerr << "error: faidx error, len==0" << std::endl << "start: " << start << " end: " << std::endl;
                stats.dropped++;
                continue;
            }
            j.hap = j.ref;
            const int pos = int(id.refpos) - start;           // start is not clamped: near a target's first base this is not where the indel is
            const int testlen = id.len > 0 ? 0 : -id.len;
            if (j.hap.size() < size_t(pos + testlen)) {
                std::cerr << "Cannot align variant " << id.refpos << " " << id.len << " " << id.seq << std::endl;
                stats.dropped++;
                continue;
            }
            if (id.len < 0) j.hap.erase(size_t(pos), size_t(-id.len));
            else if (id.len > 0) j.hap.insert(size_t(pos), id.seq);
            (width == kAlignWindow ? narrow : wide).push_back(jobs.size());
            jobs.push_back(j);
        }
    }
    // one launch per batch; the candidates with a wider window go into batches of their own (the longest pair sizes every tile of a launch)
    std::vector<Found> results(nCand);
    for (int pass = 0; pass < 2; pass++) {
        const std::vector<size_t> &list = pass ? wide : narrow;
        for (size_t a = 0; a < list.size(); a += size_t(opt.batchCandidates)) {
            const size_t e = std::min(list.size(), a + size_t(opt.batchCandidates));
            runBatch(jobs, std::vector<size_t>(list.begin() + long(a), list.begin() + long(e)), opt, stats, results);
        }
    }
    // in candidate order: a variant's count is assigned, the last candidate that lands on it wins (:224)
    std::map<int, std::map<std::string, int> > realigned;
    for (size_t c = 0; c < nCand; c++)
        for (size_t v = 0; v < results[c].size(); v++) realigned[results[c][v].first][results[c][v].second] = counts[c];
    for (std::map<int, std::map<std::string, int> >::const_iterator it = realigned.begin(); it != realigned.end(); ++it) {
        std::ostringstream ovar, ocnt;
        ovar << tid << " " << it->first;
        for (std::map<std::string, int>::const_iterator v = it->second.begin(); v != it->second.end(); ++v) { ovar << " " << v->first; ocnt << " " << v->second; }
        out << ovar.str() << " #" << ocnt.str() << std::endl;
    }
}

// reference GetCandidates.cpp:305-386
void outputLibraries(LibraryInsertSizes &libs, std::ostream &out, bool quiet)
{
    for (LibraryInsertSizes::iterator lib = libs.begin(); lib != libs.end(); ++lib) {
        InsertSizes &sizes = lib->second;
        long tot = 0;
        std::set<int> ordered;
        for (InsertSizes::const_iterator it = sizes.begin(); it != sizes.end(); ++it) { tot += it->second; ordered.insert(it->first); }
        double cum = 0;
        const int median = int(tot / 2);
        int medianSize = -1;
        for (std::set<int>::const_iterator it = ordered.begin(); it != ordered.end(); ++it) {
            cum += double(sizes[*it]);
            if (medianSize == -1 && cum > median) medianSize = *it;
        }
        const int maxSize = medianSize * 10;
        const double dtot = double(tot);
        double mean = 0.0, var = 0.0;
        for (InsertSizes::const_iterator it = sizes.begin(); it != sizes.end(); ++it)
            if (it->first < maxSize) mean += double(it->first) * double(it->second) / dtot;
        for (InsertSizes::const_iterator it = sizes.begin(); it != sizes.end(); ++it)
            if (it->first < maxSize) { const double dist = double(it->first) - mean; var += double(it->second) / dtot * dist * dist; }
        if (!quiet) std::cout << "Library: " << lib->first << " mean: " << mean << " stddev: " << sqrt(var) << std::endl;
        const int len = int(mean + 5 * sqrt(var));
        std::vector<long> histo(size_t(len > 0 ? len : 0), 2), smooth(size_t(len > 0 ? len : 0), 2);
        for (InsertSizes::const_iterator it = sizes.begin(); it != sizes.end(); ++it)
            if (it->first >= 0 && it->first < len) histo[size_t(it->first)] = it->second;
        const int L = 5;
        for (int i = 0; i < len; i++) {
            const int lo = i - L < 0 ? 0 : i - L, hi = i + L > len ? len : i + L;     // [i - 5, i + 5): the upper bound is not symmetric
            int n = 0;
            long sum = 0;
            for (int j = lo; j < hi; j++, n++) sum += histo[size_t(j)];
            smooth[size_t(i)] = (sum + 1) / (n + 1);
        }
        out << "#LIB " << lib->first << std::endl;
        for (int i = 0; i < len; i++) out << i << " " << smooth[size_t(i)] << std::endl;
    }
}

namespace {

// the pairs whose insert size counts (:447) and the library they count for (:448-451).  `fallback` starts as "dindel_default" and — as in
// the reference, where `lib` is a reference to that string and is assigned through — becomes the last library name seen, so a record
// without a library behind one with a library is counted for that library.
void countInsertSize(const BamFile &bam, const BamRecord &b, std::string &fallback, LibraryInsertSizes &libs)
{
    if (!(b.flag & BAM_FPAIRED) || !(b.flag & BAM_FPROPER_PAIR) || b.tid != b.mtid || (b.flag & (BAM_FDUP | BAM_FQCFAIL))) return;
    const char *p = bam.getLibrary(b);
    if (p) fallback = p;
    InsertSizes &sizes = libs[fallback];
    const int isize = std::abs(b.isize);
    InsertSizes::iterator it = sizes.find(isize);
    if (it == sizes.end()) sizes[isize] = 1; else it->second += 1;
}

void addRecord(const BamFile &bam, CandidateTable &table)
{
    const std::vector<uint8_t> &raw = bam.rawRecord();
    std::vector<CigarIndel> indels;
    cigarIndels(RawBamView(raw.data(), raw.size()), indels);
    for (size_t i = 0; i < indels.size(); i++) addCandidate(table, indels[i]);
}

} // namespace

// reference GetCandidates.cpp:387-486
void candidatesFromBam(const std::string &bamFile, const std::string &outputFile, IndexedFasta &fa, const CandidateOptions &opt, CandidateStats &stats)
{
    BamFile bam(bamFile);
    const std::string variantsName = outputFile + ".variants.txt", librariesName = outputFile + ".libraries.txt";
    std::ofstream out(variantsName.c_str());
    if (!out.is_open()) throw std::string("Cannot open ").append(outputFile).append(" for writing CIGAR indels.");
    if (!opt.quiet) std::cout << "Parsing indels from CIGAR strings..." << std::endl;
    CandidateTable table;
    LibraryInsertSizes libs;
    std::string fallback("dindel_default"), oldName;
    int oldTid = -1;
    BamRecord b;
    while (bam.next(b)) {
        if (b.tid < 0 || size_t(b.tid) >= bam.targetNames().size()) continue;          // unmapped
        if (b.tid != oldTid) {
            if (oldTid != -1) {
                outputIndels(oldName, table, out, fa, opt, stats);
                if (!opt.quiet) std::cout << "Wrote indels in CIGARS for target " << oldName << " to file " << outputFile << std::endl;
            }
            oldTid = b.tid; oldName = bam.targetNames()[size_t(b.tid)];
            table.clear();
        }
        addRecord(bam, table);
        countInsertSize(bam, b, fallback, libs);
    }
    outputIndels(oldName, table, out, fa, opt, stats);
    std::ofstream lout(librariesName.c_str());
    if (!lout.is_open()) throw std::string("Cannot open ").append(librariesName).append(" for writing libraries.");
    outputLibraries(libs, lout, opt.quiet);
    if (!opt.quiet)
        std::cout << "Wrote indels in CIGARS for target " << oldName << " to file " << outputFile << std::endl
                  << "Wrote library insert sizes to " << librariesName << std::endl << "done!" << std::endl;
}

// reference GetCandidates.cpp:50-62
void candidatesFromRegion(const std::vector<std::string> &bamFiles, const std::string &tid, int start, int end, const std::string &outputFile,
                          IndexedFasta &fa, const CandidateOptions &opt, CandidateStats &stats)
{
    CandidateTable table;
    for (size_t f = 0; f < bamFiles.size(); f++) {
        BamFile bam(bamFiles[f]);
        BamFile *bp = &bam;
        CandidateTable *tp = &table;
        bam.fetchCore(bam.getTID(tid), start, end, [bp, tp](BamRecord &) { addRecord(*bp, *tp); return true; });
    }
    std::ofstream out(outputFile.c_str());
    if (!out.is_open()) throw std::string("Cannot open variants file ").append(outputFile).append(" for writing.");
    outputIndels(tid, table, out, fa, opt, stats);
}

// reference GetCandidates.cpp:260-303; the lines are those of VariantFile::getLine (VariantFile.hpp:120-186): `tid pos variant ...`, ended
// by the first word that does not start like a variant (the `#` in front of the counts)
void realignCandidateFile(const std::string &varFile, bool isOneBased, const std::string &outputFile, IndexedFasta &fa,
                          const CandidateOptions &opt, CandidateStats &stats)
{
    std::ifstream in(varFile.c_str());
    if (!in.is_open()) throw std::string("Cannot open variant file ").append(varFile);
    std::ofstream out(outputFile.c_str());
    if (!out.is_open()) throw std::string("Cannot open ").append(outputFile).append(" for writing CIGAR indels.");
    if (!opt.quiet) std::cout << "Realigning indels from variants file: " << varFile << std::endl;
    CandidateTable table;
    std::string current, line;
    int index = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        index++;
        const std::vector<std::string> words = splitWords(line);
        if (words.size() < 2) continue;
        long pos = strtol(words[1].c_str(), NULL, 10);
        if (isOneBased) pos--;
        std::vector<AlignedVariant> variants;
        bool bad = false;
        for (size_t k = 2; k < words.size() && !bad; k++) {
            if (!strchr("-+ACGTR", words[k][0])) break;
            try {
                AlignedVariant v(words[k], int(pos));
                if (!v.getSeq().empty()) variants.push_back(v);
            } catch (const std::string &) { bad = true; }
        }
        if (bad) { std::cerr << "Could not parse variants in line " << index << " in variants file." << std::endl; continue; }
        if (variants.empty()) { std::cerr << "Could not parse any variants in line: " << index << " SKIPPING." << std::endl; continue; }
        if (words[0] != current) {
            if (table.size()) {
                outputIndels(current, table, out, fa, opt, stats);
                if (!opt.quiet) std::cout << "Wrote realigned candidate indel for target " << current << " to file " << outputFile << std::endl;
            }
            table.clear();
            current = words[0];
        }
        for (size_t v = 0; v < variants.size(); v++) if (variants[v].isIndel()) {
            const int len = variants[v].getType() == AlignedVariant::DEL ? -variants[v].size() : variants[v].size();
            addCandidate(table, CigarIndel(uint32_t(pos), len, variants[v].getSeq()));
        }
    }
    outputIndels(current, table, out, fa, opt, stats);
    if (!opt.quiet) std::cout << "Wrote realigned candidate indels for target " << current << " to file " << outputFile << std::endl;
}

namespace {

const char *kUsage =
    "usage: dindel_candidates --analysis getCIGARindels|realignCandidates --ref FASTA --outputFile OUT [options]\n"
    "  --analysis getCIGARindels     candidate indels from the CIGARs of a BAM file, realigned to their canonical position\n"
    "      --bamFile FILE            whole file: writes OUT.variants.txt and OUT.libraries.txt\n"
    "      --bamFiles LIST           a file naming one BAM file per line (region runs only)\n"
    "      --tid NAME --region A-B   only records overlapping [A, B) of target NAME: writes OUT itself\n"
    "  --analysis realignCandidates  realign the indels of a `tid pos variant ... # ...` file: writes OUT.variants.txt\n"
    "      --varFile FILE            the candidates; --varFileIsOneBased: its positions are one-based\n"
    "  --ref FASTA                   reference sequence, with FASTA.fai\n"
    "  --device D                    GPU ordinal (default 0)\n"
    "  --batchCandidates N           candidates per device launch (default 65536)\n"
    "  --eventsCap N                 indel events kept per alignment on the device (default 8); an alignment with more is redone on the host\n"
    "  --hostConvert                 copy every alignment back and convert it on the host instead of reading its events from the device\n"
    "  --quiet                       no progress on stdout\n"
    "  --help                        this text\n";

} // namespace

void parseRegion(const std::string &region, int &start, int &end)          // reference DInDel.cpp:3892-3905
{
    std::string filtered;
    for (size_t x = 0; x < region.size(); x++) { if (region[x] == '-') filtered += ' '; else if (region[x] != ',') filtered += region[x]; }
    const std::vector<std::string> w = splitWords(filtered);
    std::istringstream a(w.size() > 0 ? w[0] : std::string()), b(w.size() > 1 ? w[1] : std::string());
    if (!(a >> start)) throw std::string("Cannot parse region for start!");
    if (!(b >> end)) throw std::string("Cannot parse region end!");
}

// the option checks, their order, messages and exit codes: reference DInDel.cpp:4188-4298
int candidatesMain(int argc, char **argv, AlignHook hook, void *hookData)
{
    std::map<std::string, std::string> val;
    std::set<std::string> flag;
    static const char *const withValue[] = {"analysis", "bamFile", "bamFiles", "ref", "outputFile", "tid", "region", "varFile", "device", "batchCandidates", "eventsCap"};
    static const char *const withoutValue[] = {"varFileIsOneBased", "hostConvert", "quiet"};
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--help" || a == "-h") { std::cout << kUsage; return 0; }
        const std::string name = a.size() > 2 && a[0] == '-' && a[1] == '-' ? a.substr(2) : std::string();
        bool known = false;
        for (size_t k = 0; k < sizeof(withValue) / sizeof(*withValue) && !known; k++)
            if (name == withValue[k] && i + 1 < argc) { val[name] = argv[++i]; known = true; }
        for (size_t k = 0; k < sizeof(withoutValue) / sizeof(*withoutValue) && !known; k++)
            if (name == withoutValue[k]) { flag.insert(name); known = true; }
        if (!known) { std::cout << "Error parsing input options. Usage: \n\n" << kUsage << "\n"; return 1; }
    }
    if (!val.count("analysis")) { std::cerr << "Error: Specify which analysis (--analysis) is required." << std::endl; return 1; }
    if (!(val.count("ref") && val.count("outputFile"))) {
        std::cerr << "Error: One of the following options was not specified:  --ref --tid or --outputFile" << std::endl;
        return 1;
    }
    CandidateOptions opt;
    opt.hook = hook; opt.hookData = hookData;
    opt.quiet = flag.count("quiet") != 0;
    opt.hostConvert = flag.count("hostConvert") != 0;
    if (val.count("device")) opt.device = atoi(val["device"].c_str());
    if (val.count("batchCandidates")) opt.batchCandidates = atoi(val["batchCandidates"].c_str());
    if (val.count("eventsCap")) opt.eventsCap = atoi(val["eventsCap"].c_str());
    if (opt.batchCandidates < 1) { std::cerr << "dindel_candidates: --batchCandidates must be at least 1" << std::endl; return 2; }
    if (opt.eventsCap < 1 || opt.eventsCap > DD_ALIGN_EVENTS_MAX_CAP) { std::cerr << "dindel_candidates: --eventsCap must be 1 ... 4096" << std::endl; return 2; }
    const std::string analysis = val["analysis"], outputFile = val["outputFile"];
    CandidateStats stats;
    try {
        if (analysis == "getCIGARindels") {
            if (!(val.count("bamFile") || val.count("bamFiles"))) { std::cerr << "Error: Specify either --bamFile or --bamFiles." << std::endl; return 1; }
            if (val.count("region") && !val.count("tid")) {
                std::cerr << "--tid must be specified if analysis==getCIGARindels and --region option is used. " << std::endl;
                return 1;
            }
            if (!val.count("region") && !val.count("bamFile")) {
                std::cerr << "Can extract the full set of indels from only BAM file at a time." << std::endl;
                return 1;
            }
            if (val.count("bamFile") && !opt.quiet) std::cout << "Reading BAM file: " << val["bamFile"] << std::endl;
            IndexedFasta fa(val["ref"]);
            if (val.count("region")) {
                int start = 0, end = 0;
                parseRegion(val["region"], start, end);
                std::vector<std::string> bams;
                if (val.count("bamFile")) bams.push_back(val["bamFile"]);
                else {
                    std::ifstream list(val["bamFiles"].c_str());
                    if (!list.is_open()) throw std::string("Cannot open file with BAM files.");
                    std::string line;
                    while (std::getline(list, line)) { const std::vector<std::string> w = splitWords(line); if (!w.empty()) bams.push_back(w[0]); }
                }
                if (!opt.quiet) std::cout << "Getting indels from CIGARs in mapped reads from region " << val["tid"] << ":" << start << "-" << end << std::endl;
                candidatesFromRegion(bams, val["tid"], start, end, outputFile, fa, opt, stats);
            } else candidatesFromBam(val["bamFile"], outputFile, fa, opt, stats);
        } else if (analysis == "realignCandidates") {
            const std::string out = outputFile + ".variants.txt";
            if (!val.count("varFile")) { std::cerr << "Please specify the file with the candidate variants." << std::endl; return 1; }
            if (val["varFile"] == out) { std::cerr << "outputFile is same as variant file used for input!" << std::endl; return 1; }
            IndexedFasta fa(val["ref"]);
            realignCandidateFile(val["varFile"], flag.count("varFileIsOneBased") != 0, out, fa, opt, stats);
        } else { std::cerr << "Unrecognized --analysis option." << std::endl; return 1; }
    } catch (const std::string &s) {
        std::cout << "Exception: " << s << std::endl;
        return 1;
    }
    if (!opt.quiet)
        std::cerr << "dindel_candidates: " << stats.candidates << " candidates in " << stats.batches << " launches, " << stats.dropped << " dropped ("
                  << stats.tooLong << " too long for the device), " << stats.overflowed << " redone on the host" << std::endl;
    return 0;
}

} // namespace dindel
