"""An independent Python restatement of everything around the EM loop of estimateHaplotypeFrequenciesBayesEM (reference DInDel.cpp:2103-2816):
active sets, priors, masks, logz, haplotype frequencies, per-variant posterior and frequency, the marginalised pair prior, per-pool genotype
likelihoods, msq, strand counts and the cells of the .glf.txt lines.  The loop itself (:2412-2543) is the library's dd_pooled_em_host
(checked against exact arithmetic in tests/test_pooled_em_cpu.py); the rest uses Python's math (glibc) in the reference's term order.

A window: dict(index, tid, left, right, cand_pos, pools, cands=[(pos, str, freq)], haps=[dict(filtered, vars={key: str})],
reads=[dict(pool, reverse, mapq (probability), unmapped)], ll[h][r], off_hap[h][r], covered={(h, r, pos, snp)}, varcov={(pos, str): (nf, nr)}).
"""
import math

import numpy as np

from dindel_tgi_amd import pooled

INF = float("inf")


def add_logs(a, b):
    if a == -INF:
        return b
    return a + math.log(1.0 + math.exp(b - a)) if a > b else b + math.log(1.0 + math.exp(a - b))


def kind_of(s):
    if s == "*REF":
        return "REF"
    if s[0] == "-":
        return "DEL"
    if s[0] == "+":
        return "INS"
    assert len(s) == 4 and s[1:3] == "=>", s
    return "SNP"


def counts(s):
    return kind_of(s) != "REF" and not (kind_of(s) == "SNP" and s[3] == "D")


def find_candidate(cands, pos, s):
    k = kind_of(s)
    for c in cands:
        if kind_of(c[1]) != k or c[0] != pos:
            continue
        if (k == "SNP" and c[1][1:4] == s[1:4]) or (k == "INS" and c[1] == s) or (k == "DEL" and len(c[1]) == len(s)):
            return c
    return None


def g(x):
    return "%g" % x


def window_lines(w, program, a0=0.001, tol=1e-4, prior_snp=1e-3, prior_indel=1e-4):
    """The window's pooled lines as dicts column -> text (only the columns the analysis sets)."""
    haps, reads, ll, left = w["haps"], w["reads"], w["ll"], w["left"]
    nh, nr = len(haps), len(reads)
    var_sets = [tuple(sorted((k, s) for k, s in h["vars"].items() if counts(s))) for h in haps]
    all_vars = sorted(set(v for vs in var_sets for v in vs))
    if program == "all":
        active = [tuple(all_vars)]
    elif program == "singlevariant":
        active = sorted(set(vs for h, vs in zip(haps, var_sets) if not h["filtered"]))
    elif program == "priorpersite":
        active = [()]
        for pos in sorted(set(v[0] for v in all_vars)):
            site = [v for v in all_vars if v[0] == pos]
            active += [tuple(sorted(set(a) | set(site))) for a in list(active)]
    else:
        raise ValueError("Unknown EM option")

    def prior_term(v):
        lnf = math.log(prior_snp) if kind_of(v[1]) == "SNP" else math.log(prior_indel)
        c = find_candidate(w["cands"], v[0] + left, v[1])
        return lnf if c is None or c[2] < 0 else math.log(c[2])
    logpriors, masks = [], []
    for a in active:
        lp = 0.0
        for v in a:
            if kind_of(v[1]) == "SNP":
                lp += prior_term(v)
        for v in a:
            if kind_of(v[1]) != "SNP":
                lp += prior_term(v)
        logpriors.append(lp)
        masks.append([int(not h["filtered"] and all(v in a for v in vs)) for h, vs in zip(haps, var_sets)])
    who, wro = np.array([0, nh], np.int32), np.array([0, nr], np.int32)
    flat = np.array([ll[h][r] for h in range(nh) for r in range(nr)], np.float64)
    em = pooled.em_host(who, wro, flat, pooled.pack_slots(who, [0] * len(active), masks), a0=a0, tol=tol) if active else None
    logliks = [float(x) for x in em["loglik"]] if active else []
    freqs = [[float(em["freqs"][a * nh + h]) for h in range(nh)] for a in range(len(active))]
    logz = -INF
    for a in range(len(active)):
        logz = add_logs(logz, logliks[a] + logpriors[a])
    hap_freqs = [0.0] * nh
    for a in range(len(active)):
        for h in range(nh):
            hap_freqs[h] += math.exp(logliks[a] + logpriors[a] - logz) * freqs[a][h]
    has = [[int(haps[h]["vars"].get(v[0]) == v[1]) for v in all_vars] for h in range(nh)]
    unmapped_realigned = sum(1 for r in range(nr) if not all(w["off_hap"][h][r] for h in range(nh)) and reads[r]["unmapped"])
    by_pool = [[r for r in range(nr) if reads[r]["pool"] == b] for b in range(w["pools"])]
    lines = []
    for vi, v in enumerate(all_vars):
        logp, freq = -INF, 0.0
        for a in range(len(active)):
            if v in active[a]:
                logp = add_logs(logp, logliks[a] + logpriors[a])
        for h in range(nh):
            if has[h][vi]:
                freq += hap_freqs[h]
        logp -= logz
        if find_candidate(w["cands"], v[0] + left, v[1]) is None:
            continue
        # haplotypes equal in every other variant share a marginal state
        states, otn = {}, []
        for h in range(nh):
            key = tuple(has[h][y] for y in range(len(all_vars)) if y != vi)
            otn.append(states.setdefault(key, len(states)))
        mar = [0.0] * len(states)
        for h in range(nh):
            mar[otn[h]] += hap_freqs[h]
        mar = [-50 if m < 1e-16 else math.log(m) for m in mar]
        snp = kind_of(v[1]) == "SNP"
        for b in range(w["pools"]):
            mine = by_pool[b]
            lik, msq, nf, nrv = [0.0, 0.0, 0.0], 0.0, 0, 0
            if mine:
                lik = [-INF] * 3
                for h1 in range(nh):
                    for h2 in range(h1, nh):
                        t = mar[otn[h1]] + mar[otn[h2]]
                        for r in mine:
                            t += math.log(0.5) + add_logs(ll[h1][r], ll[h2][r])
                        geno = has[h1][vi] + has[h2][vi]
                        lik[geno] = add_logs(lik[geno], t)
                for r in mine:
                    ml = max(ll[h][r] for h in range(nh))
                    best = [h for h in range(nh) if ll[h][r] >= ml - 1e-7]
                    hit = any(has[h][vi] and (h, r, v[0], int(snp)) in w["covered"] for h in best)
                    nf += int(hit and not reads[r]["reverse"])
                    nrv += int(hit and reads[r]["reverse"])
                    mq = -10 * math.log10(1.0 - reads[r]["mapq"])
                    msq += mq * mq
                msq = math.sqrt(msq / len(mine))
            cov = w["varcov"].get(v, (0, 0))
            row = dict(msg="ok", index=str(w["index"]), tid=w["tid"], analysis_type=program, indidx=str(b), was_candidate_in_window="1", lpos=str(left),
                       rpos=str(w["right"]), center_position=str(w["cand_pos"]), realigned_position=str(v[0] + left), post_prob_variant=g(math.exp(logp)),
                       est_freq=g(freq), logZ=g(logz), nref_all=v[1], num_reads=str(len(mine)), msq=g(msq), num_cover_forward=str(nf), num_cover_reverse=str(nrv),
                       num_unmapped_realigned=str(unmapped_realigned), var_coverage_forward=str(cov[0]), var_coverage_reverse=str(cov[1]),
                       glf="0/0:%s;0/1:%s;1/1:%s" % tuple(g(x) for x in lik))
            if b == 0:
                parts = []
                for h in range(nh):
                    if nr and hap_freqs[h] > 1.0 / (2 * nr):
                        vs = ["%d,%s" % (left + k, s) for k, s in sorted(haps[h]["vars"].items()) if s != "*REF"]
                        parts.append((",".join(vs) if vs else "REF") + ":" + g(hap_freqs[h]))
                row["hapfreqs"] = ";".join(parts)
            lines.append(row)
    return lines


def window_text(w):
    """The window in the records of host/pooled_em_text.hpp."""
    out = ["W %d %s %d %d %d %d" % (w["index"], w["tid"], w["left"], w["right"], w["cand_pos"], w["pools"])]
    out += ["C %d %s %.17g" % c for c in w["cands"]]
    for h in w["haps"]:
        out.append("H %d" % int(h["filtered"]))
        out += ["V %d %s" % (k, s) for k, s in sorted(h["vars"].items())]
    out += ["R %d %d %.17g %d" % (r["pool"], int(r["reverse"]), r["mapq"], int(r["unmapped"])) for r in w["reads"]]
    for h in range(len(w["haps"])):
        for r in range(len(w["reads"])):
            out.append("L %d %d %.17g %d" % (h, r, w["ll"][h][r], int(w["off_hap"][h][r])))
    out += ["K %d %d %d %d" % k for k in sorted(w["covered"])]
    out += ["X %d %s %d %d" % (k[0], k[1], v[0], v[1]) for k, v in sorted(w["varcov"].items())]
    return "\n".join(out) + "\n"
