// haplotypes.cpp — see haplotypes.hpp.  Reference: HaplotypeDistribution.cpp:29-45, 74-164, 179-436; HapBlock.cpp:20-81;
// HaplotypeDistribution.hpp:85-116, 171-309, 312-482; DInDel.cpp:1526-1592.
#include "haplotypes.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <set>
#include <sstream>

namespace dindel {

namespace {

enum { OP_M = 0, OP_I = 1, OP_D = 2, OP_N = 3, OP_S = 4, OP_H = 5 };
const int kMaxCodedDeletion = 30;      // HaplotypeDistribution.cpp:127-131: a longer deletion is coded, and advances, as 30

inline bool takesLetters(int op) { return op == OP_M || op == OP_I || op == OP_S; }
inline int advanceOf(int op, int len) { return (op == OP_M || op == OP_N) ? len : op == OP_D ? std::min(len, kMaxCodedDeletion) : 0; }
inline bool knownOp(int op) { return op >= OP_M && op <= OP_H; }

// the offsets of window w and of its reads, checked as the kernel checks them
struct WindowView {
    int rs, ro, L, r0, r1;
    bool sane;
    WindowView(const dd_hap_batch &b, int w)
    {
        rs = b.win_rs[w]; ro = b.win_ref_off[w]; L = b.win_ref_off[w + 1] - ro; r0 = b.win_read_off[w]; r1 = b.win_read_off[w + 1];
        sane = rs >= 0 && ro >= 0 && ro + L <= b.win_ref_off[b.n_windows] && r0 >= 0 && r1 >= r0 && r1 <= b.n_reads;
    }
};

struct ReadView {
    int o0, o1, b0, nb; int64_t pos; int flag;
    bool sane;
    ReadView(const dd_hap_batch &b, int r)
    {
        o0 = b.read_op_off[r]; o1 = b.read_op_off[r + 1]; b0 = b.read_base_off[r]; nb = b.read_base_off[r + 1] - b0;
        pos = b.read_pos[r]; flag = b.read_flag[r];
        const int totOps = b.read_op_off[b.n_reads], totBases = b.read_base_off[b.n_reads];
        sane = o0 >= 0 && o1 >= o0 && o1 <= totOps && o1 - o0 <= 65535 && b0 >= 0 && nb >= 0 && nb <= totBases - b0;
    }
};

// a block's strings while they are collected: key (bytes big-endian, left-aligned) -> count; std::map orders keys as the strings order
typedef std::map<uint32_t, uint32_t> KeyCounts;

uint32_t keyOf(const char *p, int n)
{
    uint32_t k = 0;
    for (int j = 0; j < n; j++) k |= uint32_t((unsigned char)p[j]) << (24 - 8 * j);
    return k;
}

void setFrequencies(HapBlockTable &hb)
{
    int sum = 0;
    for (size_t i = 0; i < hb.entries.size(); i++) sum += hb.entries[i].count;
    for (size_t i = 0; i < hb.entries.size(); i++) hb.entries[i].freq = double(hb.entries[i].count) / double(sum);
}

} // namespace

void HapBatchData::addRead(int32_t pos, int32_t flag, const uint32_t *cigar, size_t nCigar, const std::string &letters)
{
    readPos.push_back(pos); readFlag.push_back(flag);
    ops.insert(ops.end(), cigar, cigar + nCigar);
    readOpOff.push_back(int32_t(ops.size()));
    bases += letters;
    readBaseOff.push_back(int32_t(bases.size()));
    winReadOff.back() = int32_t(readPos.size());
}

dd_hap_batch HapBatchData::batch() const
{
    static const int32_t none32 = 0; static const uint32_t noneU = 0;
    dd_hap_batch b;
    b.n_windows = nWindows(); b.n_reads = int32_t(readPos.size());
    b.win_rs = winRs.empty() ? &none32 : winRs.data(); b.win_ref_off = winRefOff.data(); b.ref_seq = refSeq.c_str();
    b.win_read_off = winReadOff.data();
    b.read_pos = readPos.empty() ? &none32 : readPos.data(); b.read_flag = readFlag.empty() ? &none32 : readFlag.data();
    b.read_op_off = readOpOff.data(); b.ops = ops.empty() ? &noneU : ops.data();
    b.read_base_off = readBaseOff.data(); b.bases = bases.c_str();
    return b;
}

void HapTablesData::size(const dd_hap_batch &b)
{
    const size_t W = size_t(b.n_windows);
    blkOff.assign(W + 1, 0); entOff.assign(W + 1, 0); insOff.assign(W + 1, 0);
    if (dd_hap_blocks_offsets(&b, blkOff.data(), entOff.data(), insOff.data()) != DD_SUCCESS) throw std::string("dd_hap_blocks_offsets: ").append(dd_last_error());
    perWindow.assign(6 * std::max<size_t>(W, 1), 0);
    blocks.assign(std::max<size_t>(size_t(blkOff[W]), 1), 0); entries.assign(2 * std::max<size_t>(size_t(entOff[W]), 1), 0);
    insOps.assign(2 * std::max<size_t>(size_t(insOff[W]), 1), 0); insPos.assign(2 * std::max<size_t>(size_t(insOff[W]), 1), 0);
}

dd_hap_blocks HapTablesData::tables()
{
    const size_t W = std::max<size_t>(blkOff.size() - 1, 1);
    dd_hap_blocks t;
    int32_t *p = perWindow.data();
    t.status = p; t.n_blocks = p + W; t.n_entries = p + 2 * W; t.n_ins_ops = p + 3 * W; t.n_ins_pos = p + 4 * W; t.left = p + 5 * W;
    t.blk_off = blkOff.data(); t.ent_off = entOff.data(); t.ins_off = insOff.data();
    t.blocks = blocks.data(); t.entries = entries.data(); t.ins_ops = insOps.data(); t.ins_pos = insPos.data();
    return t;
}

// ---- the closed form ------------------------------------------------------------------------------------------------------------------
// Cuts at every 4th position from rs, at every segment's first position and behind its last; per block the distinct strings of the
// segments that cover it, counted.  Insertion positions in the order their first I comes by, each with the later crossings.

void blockTableHost(const dd_hap_batch &b, dd_hap_blocks &t)
{
    const char *ref = b.ref_seq;
    for (int w = 0; w < b.n_windows; w++) {
        const WindowView W(b, w);
        const int64_t bo = t.blk_off[w], bcap = int64_t(t.blk_off[w + 1]) - bo, eo = t.ent_off[w], ecap = int64_t(t.ent_off[w + 1]) - eo,
                      io = t.ins_off[w], icap = int64_t(t.ins_off[w + 1]) - io;
        if (W.L > DD_HAPDIST_MAX_WINDOW) { t.status[w] = DD_HAPDIST_TOO_WIDE; continue; }
        if (W.L <= 0 || !W.sane) { t.status[w] = DD_HAPDIST_HOST; continue; }
        if (bcap < 0 || ecap < 0 || icap < 0) { t.status[w] = DD_HAPDIST_OVERFLOW; continue; }
        const int L = W.L;

        // one pass over the reads for the cuts and for what the reference throws on
        std::vector<char> cut(size_t(L) + 1, 0);
        for (int p = 0; p < L; p += 4) cut[size_t(p)] = 1;
        cut[size_t(L)] = 1;
        bool host = false;
        int left = 0;
        for (int r = W.r0; r < W.r1 && !host; r++) {
            const ReadView R(b, r);
            if (R.flag & 8) continue;
            if (!R.sane || (R.pos < 0 && R.o1 > R.o0)) { host = true; break; }
            int64_t at = R.pos, before = at, used = 0;
            int prev = -1;
            for (int k = R.o0; k < R.o1; k++) {
                const int op = int(b.ops[k] & 15u), len = int(b.ops[k] >> 4);
                if (takesLetters(op) && (used += len) > R.nb) { host = true; break; }
                const int width = (op == OP_M || op == OP_S) ? len : (op == OP_D && len > 0) ? 1 : 0;
                if (width > 0) {
                    const int64_t a = at - W.rs, e = a + width;
                    if (a >= 0 && a <= L) cut[size_t(a)] = 1;
                    if (e >= 0 && e <= L) cut[size_t(e)] = 1;
                    if (a < 0) left |= e >= 0 ? 3 : 2;
                }
                if (prev != -1 && prev != OP_I && prev != OP_S && prev != OP_H && before == at) { host = true; break; }     // "Mag niet."
                if (!knownOp(op)) { host = true; break; }
                before = at; at += advanceOf(op, len); prev = op;
            }
        }
        if (host) { t.status[w] = DD_HAPDIST_HOST; continue; }

        std::vector<int> starts, blockAt(size_t(L), 0);
        for (int p = 0; p < L; p++) { if (cut[size_t(p)]) starts.push_back(p); blockAt[size_t(p)] = int(starts.size()) - 1; }
        const int nBlocks = int(starts.size());
        starts.push_back(L);
        std::vector<KeyCounts> table;
        table.resize(size_t(nBlocks));
        for (int k = 0; k < nBlocks; k++) table[size_t(k)][keyOf(ref + W.ro + starts[size_t(k)], starts[size_t(k) + 1] - starts[size_t(k)])] = 1;

        // the second pass: strings, insertion operations and crossings, in (read, operation) order
        std::vector<uint32_t> insOps, insPos;      // as in dd_hap_blocks, two words per record
        for (int r = W.r0; r < W.r1; r++) {
            const ReadView R(b, r);
            if (R.flag & 8) continue;
            int64_t at = R.pos, used = 0;
            for (int k = R.o0; k < R.o1; k++) {
                const int op = int(b.ops[k] & 15u), len = int(b.ops[k] >> 4);
                const int64_t a = at - W.rs;
                const int width = (op == OP_M || op == OP_S) ? len : (op == OP_D && len > 0) ? 1 : 0;
                if (width > 0) {
                    const int64_t lo = std::max<int64_t>(a, 0), hi = std::min<int64_t>(a + width, L);
                    for (int k2 = lo < hi ? blockAt[size_t(lo)] : nBlocks; k2 < nBlocks && starts[size_t(k2)] < hi; k2++) {
                        const int bs = starts[size_t(k2)], n = starts[size_t(k2) + 1] - bs;
                        if (op == OP_D) { const char code = char('#' + std::min(len, kMaxCodedDeletion)); table[size_t(k2)][keyOf(&code, 1)]++; }
                        else table[size_t(k2)][keyOf(b.bases + R.b0 + used + (bs - a), n)]++;
                    }
                }
                if (op == OP_I) {
                    if (len > 0 && a >= 0 && a < L) {
                        size_t known = 0;
                        while (known < insPos.size() && insPos[known] != uint32_t(a)) known += 2;
                        if (known == insPos.size()) { insPos.push_back(uint32_t(a)); insPos.push_back(0); }
                        insOps.push_back(uint32_t(r - W.r0)); insOps.push_back((uint32_t(k - R.o0) << 16) | uint32_t(a));
                    }
                } else if (k < R.o1 - 1) {
                    const int64_t e = a + advanceOf(op, len);
                    for (size_t i = 0; i < insPos.size(); i += 2) if (int64_t(insPos[i]) >= a && int64_t(insPos[i]) < e) insPos[i + 1]++;
                }
                if (takesLetters(op)) used += len;
                at += advanceOf(op, len);
            }
        }

        size_t nEntries = 0;
        bool overflow = nBlocks > bcap || int64_t(insOps.size() / 2) > icap || insPos.size() / 2 > DD_HAPDIST_MAX_INS_POS;
        for (int k = 0; k < nBlocks; k++) { nEntries += table[size_t(k)].size(); overflow = overflow || table[size_t(k)].size() > DD_HAPDIST_MAX_DISTINCT; }
        if (overflow || int64_t(nEntries) > ecap) { t.status[w] = DD_HAPDIST_OVERFLOW; continue; }

        uint32_t *e = t.entries + 2 * eo;
        for (int k = 0; k < nBlocks; k++) {
            const int bs = starts[size_t(k)], n = starts[size_t(k) + 1] - bs;
            const uint32_t refKey = keyOf(ref + W.ro + bs, n);
            uint32_t refIdx = 0, i = 0;
            for (KeyCounts::const_iterator it = table[size_t(k)].begin(); it != table[size_t(k)].end(); ++it, ++i) {
                if (it->first == refKey) refIdx = i;
                *e++ = it->first; *e++ = it->second;
            }
            t.blocks[bo + k] = uint32_t(bs) | (uint32_t(n) << 16) | (i << 20) | (refIdx << 26);
        }
        std::copy(insOps.begin(), insOps.end(), t.ins_ops + 2 * io);
        std::copy(insPos.begin(), insPos.end(), t.ins_pos + 2 * io);
        t.n_blocks[w] = nBlocks; t.n_entries[w] = int32_t(nEntries); t.n_ins_ops[w] = int32_t(insOps.size() / 2);
        t.n_ins_pos[w] = int32_t(insPos.size() / 2); t.left[w] = left; t.status[w] = DD_HAPDIST_OK;
    }
}

WindowTable tableFromFlat(const dd_hap_batch &b, const dd_hap_blocks &t, int w)
{
    WindowTable out;
    const WindowView W(b, w);
    out.left = t.left[w];
    const uint32_t *e = t.entries + 2 * size_t(t.ent_off[w]);
    for (int k = 0; k < t.n_blocks[w]; k++) {
        const uint32_t word = t.blocks[t.blk_off[w] + k];
        const int bs = int(word & 0xffffu), n = int((word >> 16) & 15u), cnt = int((word >> 20) & 63u), refIdx = int(word >> 26);
        HapBlockTable hb;
        hb.start = uint32_t(W.rs + bs); hb.end = hb.start + uint32_t(n) - 1; hb.insertion = false;
        for (int i = 0; i < cnt; i++, e += 2) {
            BlockEntry be;
            for (int j = 0; j < n; j++) be.seq += char((e[0] >> (24 - 8 * j)) & 0xffu);
            be.count = int(e[1]); be.isRef = i == refIdx; be.freq = 0.0;
            hb.entries.push_back(be);
        }
        setFrequencies(hb);
        out.blocks.push_back(hb);
    }
    // insertion positions by position; a position's strings from the reads that carry them
    std::map<uint32_t, std::map<std::string, int> > byPos;
    std::map<uint32_t, int> crossings;
    const uint32_t *ip = t.ins_pos + 2 * size_t(t.ins_off[w]), *iop = t.ins_ops + 2 * size_t(t.ins_off[w]);
    for (int i = 0; i < t.n_ins_pos[w]; i++) { byPos[ip[2 * i]]; crossings[ip[2 * i]] = int(ip[2 * i + 1]); }
    for (int i = 0; i < t.n_ins_ops[w]; i++) {
        const int r = W.r0 + int(iop[2 * i]), kOp = int(iop[2 * i + 1] >> 16);
        const uint32_t at = iop[2 * i + 1] & 0xffffu;
        if (r < W.r0 || r >= W.r1) throw std::string("block table: insertion record names a read outside the window");
        const ReadView R(b, r);
        if (kOp >= R.o1 - R.o0) throw std::string("block table: insertion record names an operation the read does not have");
        int64_t used = 0;
        for (int k = R.o0; k < R.o0 + kOp; k++) if (takesLetters(int(b.ops[k] & 15u))) used += int(b.ops[k] >> 4);
        const int len = int(b.ops[R.o0 + kOp] >> 4);
        if (used + len > R.nb) throw std::string("block table: insertion record runs past the read's letters");
        byPos[at][std::string(b.bases + R.b0 + used, size_t(len))]++;
    }
    for (std::map<uint32_t, std::map<std::string, int> >::const_iterator it = byPos.begin(); it != byPos.end(); ++it) {
        HapBlockTable hb;
        hb.start = uint32_t(W.rs) + it->first; hb.insertion = true;
        const BlockEntry none = {std::string(), 1 + crossings[it->first], true, 0.0};
        hb.entries.push_back(none);
        size_t first = 0;
        for (std::map<std::string, int>::const_iterator s = it->second.begin(); s != it->second.end(); ++s) {
            const BlockEntry be = {s->first, s->second, false, 0.0};
            hb.entries.push_back(be);
            if (!first) first = s->first.size();
        }
        hb.end = hb.start - 1;
        setFrequencies(hb);
        out.insertions.push_back(hb);
    }
    return out;
}

// ---- the fallback: one segment after the other ------------------------------------------------------------------------------------------

namespace {

struct Seen { int count; bool isRef; };
struct Stretch { int64_t end; std::map<std::string, Seen> seen; };      // [key, end)
typedef std::map<int64_t, Stretch> Stretches;

void see(std::map<std::string, Seen> &m, const std::string &s, int times, bool isRef)
{
    std::map<std::string, Seen>::iterator it = m.find(s);
    if (it == m.end()) { const Seen n = {times, isRef}; m[s] = n; }
    else { it->second.count += times; it->second.isRef = it->second.isRef || isRef; }
}

// a boundary at x: the stretch that holds x in its inside becomes two, each string cut at x
void cutAt(Stretches &all, int64_t x)
{
    Stretches::iterator it = all.upper_bound(x);
    if (it == all.begin()) return;
    --it;
    if (it->first >= x || it->second.end <= x) return;
    Stretch right;
    right.end = it->second.end;
    std::map<std::string, Seen> leftSeen;
    const size_t n = size_t(x - it->first);
    for (std::map<std::string, Seen>::const_iterator s = it->second.seen.begin(); s != it->second.seen.end(); ++s) {
        see(leftSeen, s->first.substr(0, n), s->second.count, s->second.isRef);
        see(right.seen, s->first.size() > n ? s->first.substr(n) : std::string(), s->second.count, s->second.isRef);
    }
    it->second.end = x; it->second.seen.swap(leftSeen);
    all[x] = right;
}

void lay(Stretches &all, int64_t a, const std::string &s, bool isRef)
{
    const int64_t e = a + int64_t(s.size());
    cutAt(all, a); cutAt(all, e);
    int64_t at = a;
    Stretches::iterator it = all.lower_bound(a);
    while (at < e) {
        const int64_t upTo = (it == all.end() || it->first >= e) ? e : it->first;
        if (upTo > at) {                         // nothing here yet: one new stretch up to the next one
            Stretch fresh; fresh.end = upTo;
            see(fresh.seen, s.substr(size_t(at - a), size_t(upTo - at)), 1, isRef);
            all[at] = fresh;
            at = upTo;
            continue;
        }
        see(it->second.seen, s.substr(size_t(at - a), size_t(it->second.end - at)), 1, isRef);
        at = it->second.end;
        ++it;
    }
}

HapBlockTable blockOf(int64_t start, int64_t end, const std::map<std::string, Seen> &seen, bool insertion)
{
    HapBlockTable hb;
    hb.start = uint32_t(start); hb.end = uint32_t(end - 1); hb.insertion = insertion;
    for (std::map<std::string, Seen>::const_iterator s = seen.begin(); s != seen.end(); ++s) {
        const BlockEntry be = {s->first, s->second.count, s->second.isRef, 0.0};
        hb.entries.push_back(be);
    }
    setFrequencies(hb);
    return hb;
}

} // namespace

WindowTable sequentialTable(const dd_hap_batch &b, int w)
{
    const WindowView W(b, w);
    if (!W.sane || W.L < 0) throw std::string("block table: the window's offsets do not fit the batch");
    Stretches all;
    std::map<int64_t, std::map<std::string, Seen> > insertions;
    const std::string ref(b.ref_seq + W.ro, size_t(W.L));
    for (size_t x = 0; x < ref.size(); x += 4) lay(all, int64_t(W.rs) + int64_t(x), ref.substr(x, 4), true);
    for (int r = W.r0; r < W.r1; r++) {
        const ReadView R(b, r);
        if (R.flag & 8) continue;
        if (!R.sane) throw std::string("block table: the read's offsets do not fit the batch");
        int64_t at = R.pos, before = at, used = 0;
        int prev = -1;
        for (int k = R.o0; k < R.o1; k++) {
            const int op = int(b.ops[k] & 15u), len = int(b.ops[k] >> 4);
            std::string shown;
            if (takesLetters(op)) {
                if (used + len > R.nb) throw std::string("CIGAR longer than the read");          // the reference reads past the record here
                shown.assign(b.bases + R.b0 + used, size_t(len));
                used += len;
            } else if (op == OP_D && len > 0) shown.assign(1, char('#' + std::min(len, kMaxCodedDeletion)));
            if (!shown.empty()) {
                if (op == OP_I) {
                    std::map<int64_t, std::map<std::string, Seen> >::iterator it = insertions.find(at);
                    if (it == insertions.end()) { see(insertions[at], shown, 1, false); see(insertions[at], std::string(), 1, true); }
                    else see(it->second, shown, 1, false);
                } else lay(all, at, shown, false);
            }
            if (prev != -1 && prev != OP_I) {
                if (before == at && prev != OP_S && prev != OP_H) throw std::string("Mag niet.");
                for (std::map<int64_t, std::map<std::string, Seen> >::iterator it = insertions.lower_bound(before); it != insertions.end() && it->first < at; ++it)
                    see(it->second, std::string(), 1, false);
            }
            before = at;
            if (!knownOp(op)) throw std::string("I don't know how to smoke this CIGAR");
            at += advanceOf(op, len);
            prev = op;
        }
    }
    WindowTable out;
    out.left = 0;
    const int64_t lo = W.rs, hi = int64_t(W.rs) + W.L;
    for (Stretches::const_iterator it = all.begin(); it != all.end(); ++it) {
        if (it->first < lo) out.left |= it->second.end == lo ? 3 : 2;
        else if (it->second.end <= hi) out.blocks.push_back(blockOf(it->first, it->second.end, it->second.seen, false));
    }
    for (std::map<int64_t, std::map<std::string, Seen> >::const_iterator it = insertions.begin(); it != insertions.end(); ++it)
        if (it->first >= lo && it->first < hi) out.insertions.push_back(blockOf(it->first, it->first, it->second, true));
    return out;
}

// ---- HDIterator2 ----------------------------------------------------------------------------------------------------------------------

std::vector<HapBlockTable> selectBlocks(const WindowTable &t, uint32_t rs, uint32_t left, uint32_t right)
{
    std::vector<HapBlockTable> chosen;
    for (size_t k = 0; k < t.blocks.size(); k++) {
        const HapBlockTable &hb = t.blocks[k];
        if (hb.start < left || hb.end > right) continue;
        // the block in front: the previous one of the window, or whatever ends left of rs.  With nothing at all in front the reference
        // reads hapBlocks[-1] (undefined); that window goes on here as if the blocks were consecutive.
        const bool gap = k > 0 ? t.blocks[k - 1].end + 1 != hb.start : (hb.start != rs || ((t.left & 2) && !(t.left & 1)));
        if (gap) throw std::string("Blocks are not consecutive.");
        chosen.push_back(hb);
    }
    // each insertion position from `left` on goes in front of the first block, behind the previous insertion's place, that starts at it or later
    size_t from = 0;
    for (size_t i = 0; i < t.insertions.size(); i++) {
        const HapBlockTable &ins = t.insertions[i];
        if (ins.start < left) continue;
        for (size_t k = from; k < chosen.size(); k++) {
            if (chosen[k].start >= ins.start) {
                chosen.insert(chosen.begin() + long(k), ins);
                from = k + 1;
                break;
            }
        }
    }
    for (size_t k = 0; k < chosen.size(); k++) if (chosen[k].insertion) chosen[k].end = chosen[k].start - 1;
    if (chosen.empty()) throw std::string("Not enough blocks.");
    return chosen;
}

double setThresholds(std::vector<HapBlockTable> &hbs, size_t maxHap)
{
    struct Sum { static double of(const std::vector<HapBlockTable> &v) { double s = 0.0; for (size_t x = 0; x < v.size(); x++) s += log(double(v[x].entries.size())); return s; } };
    const double allowed = std::max(log(double(maxHap)), 0.0);
    double logNum = Sum::of(hbs);
    std::vector<double> rarest(hbs.size(), 0.0);
    std::vector<char> fixed(hbs.size(), 0);              // a block seen with one string stays marked, as the reference's elim does
    bool dropped = true;
    while (logNum > allowed && dropped) {
        dropped = false;
        for (size_t x = 0; x < hbs.size(); x++) {
            double least = 2.0;
            for (size_t y = 0; y < hbs[x].entries.size(); y++) if (!hbs[x].entries[y].isRef && hbs[x].entries[y].freq < least) least = hbs[x].entries[y].freq;
            if (hbs[x].entries.size() <= 1) { rarest[x] = 2.0; fixed[x] = 1; } else rarest[x] = least;
        }
        const size_t y = size_t(std::min_element(rarest.begin(), rarest.end()) - rarest.begin());       // the first minimum
        if (fixed[y]) break;
        std::vector<BlockEntry> &en = hbs[y].entries;
        for (size_t i = 0; i < en.size(); i++) if (!en[i].isRef && en[i].freq <= rarest[y]) { en.erase(en.begin() + long(i)); dropped = true; break; }
        logNum = Sum::of(hbs);
    }
    for (size_t x = 0; x < hbs.size(); x++) {
        bool hasRef = false;
        for (size_t y = 0; y < hbs[x].entries.size(); y++) hasRef = hasRef || hbs[x].entries[y].isRef;
        if (!hasRef) throw std::string("Cannot find reference sequence.");
    }
    return logNum;
}

namespace {

inline bool isDeletionCode(char c) { return c >= 35 && c < 65; }

struct Candidate { std::string seq; std::vector<int> at; };       // per base its reference position, -1 for an inserted one

} // namespace

std::vector<std::string> generateHaplotypes(const std::vector<HapBlockTable> &hbs, const std::vector<AlignedVariant> &variants, bool changeINStoN)
{
    std::vector<Candidate> all;
    std::vector<size_t> pick(hbs.size(), 0);
    for (bool done = hbs.empty(); !done;) {
        Candidate c;
        for (size_t x = 0; x < hbs.size(); x++) {
            const std::string &s = hbs[x].entries[pick[x]].seq;
            if (!hbs[x].insertion) {
                bool coded = false;
                for (size_t y = 0; y < s.size(); y++) { coded = coded || isDeletionCode(s[y]); c.at.push_back(int(hbs[x].start) + int(y)); }
                if (!coded && int(s.size()) != int(hbs[x].end) - int(hbs[x].start) + 1) throw std::string("What's going on here?");
            } else c.at.insert(c.at.end(), s.size(), -1);
            c.seq += s;
        }
        for (size_t y = 0; y < c.seq.size();) {          // a deletion code takes itself and what follows it away
            if (!isDeletionCode(c.seq[y])) { y++; continue; }
            const size_t n = std::min(size_t(c.seq[y] - '#'), c.seq.size() - y);
            c.seq.erase(y, n);
            c.at.erase(c.at.begin() + long(y), c.at.begin() + long(y + n));
        }
        all.push_back(c);
        size_t x = 0;                                    // the first block turns fastest
        while (x < pick.size() && ++pick[x] == hbs[x].entries.size()) { pick[x] = 0; x++; }
        done = x == pick.size();
    }
    // the variants flagged "add combinatorially" first, each on everything made so far; then the others, each on what the first round left
    for (int round = 0; round < 2; round++) {
        const bool combinatorially = round == 0;
        size_t upTo = all.size();
        for (size_t v = 0; v < variants.size(); v++) {
            const AlignedVariant &var = variants[v];
            if (combinatorially) upTo = all.size();
            if (var.getAddComb() != combinatorially) continue;
            for (size_t h = 0; h < upTo; h++) {
                const std::vector<int>::const_iterator hit = std::find(all[h].at.begin(), all[h].at.end(), var.getStartHap());
                if (hit == all[h].at.end()) continue;
                Candidate c = all[h];
                const size_t idx = size_t(hit - all[h].at.begin());
                bool changed = false;
                if (var.getType() == AlignedVariant::DEL) {
                    const size_t n = std::min(size_t(var.size()), c.seq.size() - idx);
                    c.seq.erase(idx, n);
                    c.at.erase(c.at.begin() + long(idx), c.at.begin() + long(idx + n));
                    changed = true;
                } else if (var.getType() == AlignedVariant::INS) {
                    c.seq.insert(idx, changeINStoN ? std::string(var.getSeq().size(), 'N') : var.getSeq());
                    c.at.insert(c.at.begin() + long(idx), size_t(var.size()), -1);
                    changed = true;
                } else if (var.getType() == AlignedVariant::SNP) {
                    const char to = var.getSeq()[3];
                    if (c.seq[idx] != to) { c.seq[idx] = to; changed = true; }
                }
                if (changed) all.push_back(c);
            }
        }
    }
    std::set<std::string> unique;
    for (size_t h = 0; h < all.size(); h++) unique.insert(all[h].seq);
    return std::vector<std::string>(unique.begin(), unique.end());
}

void haplotypesFromTable(const WindowTable &t, uint32_t rs, const HaplotypeOptions &opt, WindowCandidates &win)
{
    win.haps.clear(); win.message.clear(); win.returnedSkip = false; win.hapsAtSkip = 0;
    try {
        std::vector<HapBlockTable> hbs = selectBlocks(t, rs, win.leftPos, win.rightPos);
        const uint32_t start = hbs.front().start, end = hbs.back().end;
        const double logNum = setThresholds(hbs, opt.maxHap);
        if (logNum > log(double(opt.skipMaxHap))) {                                       // DInDel.cpp:1569
            std::ostringstream os; os << "too many haplotypes [>exp(" << logNum << ")]";
            win.message = os.str(); win.returnedSkip = true;
            return;
        }
        std::vector<std::string> haps = generateHaplotypes(hbs, win.variants, opt.changeINStoN);
        if (haps.size() > opt.skipMaxHap || double(haps.size() * win.nReads) > opt.maxHapReadProd) {   // DInDel.cpp:1581
            std::ostringstream os; os << "too many haplotypes [>" << haps.size() << "] numreads: " << win.nReads;
            win.message = os.str(); win.returnedSkip = true; win.hapsAtSkip = haps.size();
            return;
        }
        win.haps.swap(haps);
        win.leftPos = start; win.rightPos = end;
    } catch (std::string &e) { win.message = e; }
}

void getHaplotypesBatch(const HapBatchData &data, std::vector<WindowCandidates> &wins, const HaplotypeOptions &opt, size_t stats[2])
{
    if (int(wins.size()) != data.nWindows()) throw std::string("getHaplotypesBatch: one WindowCandidates per window");
    const dd_hap_batch b = data.batch();
    HapTablesData store;
    store.size(b);
    dd_hap_blocks t = store.tables();
    if (opt.hostDistribution) blockTableHost(b, t);
    else if (dd_hap_blocks_compute(&b, &t, opt.device) != DD_SUCCESS) throw std::string("dd_hap_blocks_compute: ").append(dd_last_error());
    for (int w = 0; w < b.n_windows; w++) {
        WindowCandidates &win = wins[size_t(w)];
        try {
            const bool ok = t.status[w] == DD_HAPDIST_OK;
            if (stats) stats[ok ? 0 : 1]++;
            const WindowTable table = ok ? tableFromFlat(b, t, w) : sequentialTable(b, w);
            haplotypesFromTable(table, uint32_t(data.winRs[size_t(w)]), opt, win);
        } catch (std::string &e) { win.haps.clear(); win.message = e; win.returnedSkip = false; win.hapsAtSkip = 0; }
    }
}

} // namespace dindel
