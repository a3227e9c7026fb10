"""TEST INFRASTRUCTURE ONLY: a Python restatement of candidate discovery (host/candidates.cpp; reference GetCandidates.cpp), written
unlike the C++: the CIGAR walk on (length, letter) tuples, the candidate table as plain dicts, alignCIGAR on top of
tests/_hapalign_oracle.py's gapped rows with the indel events read off the two rows by a column scan (not off the offset slice), the
variant lines and the library histograms.  The one thing taken as given is the order in which the reference's hash_map of positions is
walked (ddh_hash_map_order)."""
import ctypes as C
import math
import re

from tests import _hapalign_oracle as orc

INS, DEL = 1, 2
NT16 = "=ACMGRSVTWYHKDBN"


def hash_order(keys):
    from dindel_tgi_amd import hostlib
    lib = hostlib.load()
    keys = list(keys)
    arr, out = (C.c_int * max(len(keys), 1))(*keys), (C.c_int * max(len(keys), 1))()
    lib.ddh_hash_map_order.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    n = lib.ddh_hash_map_order(arr, len(keys), out)
    return list(out)[:n]


def cigar_indels(pos, cigar, seq):
    """[(refpos, len, seq)] of a record; raises ValueError with the reference's text at an operation it does not know"""
    out, ref, read = [], pos, 0
    for n, op in re.findall(r"(\d+)(.)", cigar):
        n = int(n)
        if op == "I":
            out.append((ref, n, seq[read:read + n]))
        elif op == "D":
            out.append((ref, -n, "D" * n))
        if op in "MIS":
            read += n
        if op in "MDN":
            ref += n
        if op not in "MIDNSH":
            raise ValueError("I don't know how to smoke this CIGAR")
    return out


class Table:
    """position -> {(seq, len): count}, remembering the sequence in which the positions arrived"""

    def __init__(self):
        self.at, self.arrival = {}, []

    def add(self, refpos, ln, seq):
        self.arrival.append(refpos)
        d = self.at.setdefault(refpos, {})
        d[(seq, ln)] = d.get((seq, ln), 0) + 1

    def walk(self):
        """(refpos, len, seq, count) in the reference's order: positions as its hash_map yields them, then by sequence and length"""
        for p in hash_order(self.arrival):
            for (seq, ln) in sorted(self.at[p]):
                yield p, ln, seq, self.at[p][(seq, ln)]


def events_from_rows(row0, row1):
    """(kind, ref, len, hap) of an alignment's indels, column by column: row0 the reference, row1 the haplotype"""
    hlen, rlen, n = len(row0) - row0.count("-"), len(row1) - row1.count("-"), len(row0)
    col = rb = hb = 0
    while col < n and row0[col] == "-":            # left overhang
        col += 1
        rb += 1
    out, seen = [], False
    while col < n and rb < rlen:
        if row0[col] == "-":
            if hb >= hlen:                         # right overhang
                col += 1
                rb += 1
                continue
            first = col
            while col < n and row0[col] == "-":
                col += 1
            out.append((INS, hb, col - first, rb))
            rb += col - first
        elif row1[col] == "-":
            first = col
            while col < n and row1[col] == "-":
                col += 1
            if seen:
                out.append((DEL, hb, col - first, rb))
            hb += col - first
        else:
            seen = True
            col += 1
            rb += 1
            hb += 1
    return out


def fetch(target, begin1, end1):
    begin1, end1 = max(begin1, 1), min(end1, len(target))
    return target[begin1 - 1:end1].upper() if begin1 <= end1 else ""


def make_pair(target, refpos, ln, seq):
    """(start, ref, hap) of alignCIGAR, or None where the reference drops the candidate"""
    width = 100
    if abs(ln) > width // 3:
        width = 3 * abs(ln)
    start, end = refpos - width, refpos + width
    ref = fetch(target, start + 1, end + 1)
    if not ref:
        return None
    at = refpos - start
    if len(ref) < at + (0 if ln > 0 else -ln):
        return None
    hap = ref[:at] + seq + ref[at:] if ln > 0 else ref[:at] + ref[at - ln:]
    return start, ref, hap


_aligned = {}


def align_cigar(target, refpos, ln, seq, too_long=4094):
    """[(position, '+SEQ' | '-SEQ')] of one candidate, by position"""
    pair = make_pair(target, refpos, ln, seq)
    if pair is None or max(len(pair[1]), len(pair[2])) > too_long or not pair[2]:
        return []
    start, ref, hap = pair
    if (ref, hap) not in _aligned:
        _aligned[(ref, hap)] = orc.align(ref.encode(), hap.encode())
    _, row0, row1, _ = _aligned[(ref, hap)]
    by_key = {}                                    # hap.indels is a map: a later event at a key replaces an earlier one
    r, h = row0.replace("-", ""), row1.replace("-", "")
    for kind, key, n, rb in events_from_rows(row0, row1):
        by_key[key] = "+" + h[rb:rb + n] if kind == INS else "-" + r[key:key + n]
    return [(start + k, by_key[k]) for k in sorted(by_key)]


def output_indels(tid, table, target):
    realigned = {}
    for refpos, ln, seq, count in table.walk():
        for pos, var in align_cigar(target, refpos, ln, seq):
            realigned.setdefault(pos, {})[var] = count            # assigned, not summed
    lines = []
    for pos in sorted(realigned):
        vs = sorted(realigned[pos])
        lines.append("%s %d %s # %s\n" % (tid, pos, " ".join(vs), " ".join(str(realigned[pos][v]) for v in vs)))
    return "".join(lines)


def output_libraries(libs):
    """libs: {name: [|isize| of every counted pair, in file order]}; the sections by name"""
    text = []
    for name in sorted(libs):
        counts = {}
        for s in libs[name]:
            counts[s] = counts.get(s, 0) + 1
        walk = hash_order(libs[name])
        tot = sum(counts.values())
        cum, median_size = 0, -1
        for s in sorted(counts):
            cum += counts[s]
            if median_size == -1 and cum > tot // 2:
                median_size = s
        cut = median_size * 10
        mean = 0.0
        for s in walk:
            if s < cut:
                mean += float(s) * float(counts[s]) / float(tot)
        var = 0.0
        for s in walk:
            if s < cut:
                var += float(counts[s]) / float(tot) * (float(s) - mean) * (float(s) - mean)
        n = int(mean + 5 * math.sqrt(var))
        histo = [counts[i] if i in counts else 2 for i in range(n)]
        text.append("#LIB %s\n" % name)
        for i in range(n):
            window = histo[max(i - 5, 0):min(i + 5, n)]
            text.append("%d %d\n" % (i, (sum(window) + 1) // (len(window) + 1)))
    return "".join(text)


def rg_libraries(header_text):
    out = {}
    for line in header_text.split("\n"):
        if line.startswith("@RG"):
            f = dict(x.split(":", 1) for x in line.split("\t")[1:] if ":" in x)
            if "ID" in f and "LB" in f:
                out[f["ID"]] = f["LB"]
    return out


def whole_file(header_text, names, records, targets):
    """(.variants.txt, .libraries.txt) of a whole-file run.  records: [(tid, dict)] as tests/_bamwriter.py takes them, in file order;
    targets: {name: sequence}"""
    rg = rg_libraries(header_text)
    out, libs, fallback = [], {}, "dindel_default"
    table, old = Table(), -1
    for tid, r in records:
        if tid < 0:
            continue
        if tid != old:
            if old != -1:
                out.append(output_indels(names[old], table, targets[names[old]]))
            old, table = tid, Table()
        for c in cigar_indels(r["pos"], r.get("cigar", ""), r["seq"]):
            table.add(*c)
        f = r["flag"]
        if f & 1 and f & 2 and r.get("mtid", -1) == tid and not f & (1024 | 512):
            lb = rg.get(r.get("tags", {}).get("RG"))
            if lb is not None:
                fallback = lb                      # the reference assigns through its reference to the default name
            libs.setdefault(fallback, []).append(abs(r.get("isize", 0)))
    out.append(output_indels(names[old], table, targets[names[old]]) if old != -1 else "")
    return "".join(out), output_libraries(libs)


def realign_file(text, one_based, targets):
    """realignCandidates over the text of a `tid pos variant ... # ...` file"""
    out, table, cur = [], Table(), ""
    for line in text.split("\n"):
        w = line.split()
        if len(w) < 2:
            continue
        pos = int(w[1]) - (1 if one_based else 0)
        vs = []
        for x in w[2:]:
            if x[0] not in "-+ACGTR":
                break
            vs.append(x)
        if not vs:
            continue
        if w[0] != cur:
            if table.at:
                out.append(output_indels(cur, table, targets[cur]))
            table, cur = Table(), w[0]
        for v in vs:
            if v[0] == "+":
                table.add(pos, len(v) - 1, v[1:])
            elif v[0] == "-":
                table.add(pos, -(len(v) - 1), v[1:])
    out.append(output_indels(cur, table, targets.get(cur, "")))
    return "".join(out)
