// pooled_em.cpp — see pooled_em.hpp.  Line numbers are the reference's DInDel.cpp.
#include "pooled_em.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <set>
#include <stdexcept>
#include "../../include/dindel_hmm.h"

namespace dindel {
namespace {

typedef std::set<PAV> VarSet;
typedef std::map<int, AlignedVariant>::const_iterator VarIt;

// a variant of a haplotype that counts: not the reference allele and not a "=>D" SNP (:2164)
bool counts(const AlignedVariant &v) { return !v.isRef() && !(v.isSNP() && v.getString()[3] == 'D'); }

VarSet variantsOf(const Haplotype &hap)
{
    VarSet s;
    for (VarIt it = hap.indels.begin(); it != hap.indels.end(); ++it) if (counts(it->second)) s.insert(PAV(it->first, it->second));
    return s;
}

const AlignedVariant *candidateOf(const AlignedVariant &v, uint32_t leftPos, const AlignedCandidates &cand)
{
    return cand.findVariant(int(v.getStartHap() + leftPos), v.getType(), v.getString());
}

// the prior term of one active variant (:2346-2358, :2363-2375): the candidate's frequency when the window file gives one
double priorTerm(const AlignedVariant &v, uint32_t leftPos, const AlignedCandidates &cand, const DiploidParameters &params)
{
    double lnf = 0.0;
    if (v.getType() == AlignedVariant::SNP) lnf = log(params.priorSNP);
    else if (v.getType() == AlignedVariant::DEL || v.getType() == AlignedVariant::INS) lnf = log(params.priorIndel);
    const AlignedVariant *c = candidateOf(v, leftPos, cand);
    if (!c || c->getFreq() < 0.0) return lnf;
    return log(c->getFreq());
}

std::string g6(double x)
{
    char buf[64];
    snprintf(buf, sizeof(buf), "%.6g", x);
    return buf;
}

} // namespace

bool knownBayesType(const std::string &program) { return program == "all" || program == "singlevariant" || program == "priorpersite"; }

void pooledPlan(const std::vector<Haplotype> &haps, const PooledWindow &win, uint32_t leftPos, const AlignedCandidates &candidateVariants,
                const DiploidParameters &params, const std::string &program, PooledPlan &plan)
{
    const size_t nh = haps.size();
    plan = PooledPlan();
    const std::vector<int> &filtered = win.filtered;

    VarSet all;
    std::map<int, VarSet> byPos;
    for (size_t h = 0; h < nh; h++) {
        const VarSet s = variantsOf(haps[h]);
        for (VarSet::const_iterator it = s.begin(); it != s.end(); ++it) { all.insert(*it); byPos[it->first].insert(*it); }
    }
    // the active sets; SNPs and indels of each apart, for the priors (:2172-2289)
    std::vector<VarSet> activeSets;
    if (program == "all") activeSets.push_back(all);
    else if (program == "singlevariant") {
        std::set<VarSet> distinct;
        for (size_t h = 0; h < nh; h++) if (filtered[h] == 0) distinct.insert(variantsOf(haps[h]));
        activeSets.assign(distinct.begin(), distinct.end());
    } else if (program == "priorpersite") {
        activeSets.push_back(VarSet());                                   // the reference haplotype
        for (std::map<int, VarSet>::const_iterator site = byPos.begin(); site != byPos.end(); ++site) {
            const size_t before = activeSets.size();
            for (size_t a = 0; a < before; a++) {                         // every set so far, once more with this site's SNPs and indels
                VarSet grown = activeSets[a];
                for (VarSet::const_iterator it = site->second.begin(); it != site->second.end(); ++it)
                    if (it->second.isSNP() || it->second.isIndel()) grown.insert(*it);
                activeSets.push_back(grown);
            }
        }
    } else {
        std::cerr << "Unknown EM option" << std::endl;
        exit(1);
    }
    plan.nav = int(activeSets.size());
    plan.allVariants.assign(all.begin(), all.end());
    const size_t nv = plan.allVariants.size(), nav = size_t(plan.nav);
    plan.active.assign(nav * nv, 0);
    plan.hapHasVar.assign(nh * nv, 0);
    for (size_t v = 0; v < nv; v++) {
        const PAV &pav = plan.allVariants[v];
        for (size_t a = 0; a < nav; a++) if (activeSets[a].count(pav)) plan.active[a * nv + v] = 1;
        for (size_t h = 0; h < nh; h++) {
            VarIt it = haps[h].indels.find(pav.first);
            if (it != haps[h].indels.end() && it->second.getString() == pav.second.getString()) plan.hapHasVar[h * nv + v] = 1;
        }
    }
    plan.logpriors.assign(nav, 0.0);
    plan.compat.assign(nav * nh, 0);
    for (size_t a = 0; a < nav; a++) {
        // the SNPs' terms first, then the indels', each in set order (:2343-2378); "all" and "singlevariant" keep only SNPs and indels
        double logprior = 0.0;
        for (VarSet::const_iterator it = activeSets[a].begin(); it != activeSets[a].end(); ++it)
            if (it->second.isSNP()) logprior += priorTerm(it->second, leftPos, candidateVariants, params);
        for (VarSet::const_iterator it = activeSets[a].begin(); it != activeSets[a].end(); ++it)
            if (!it->second.isSNP() && it->second.isIndel()) logprior += priorTerm(it->second, leftPos, candidateVariants, params);
        plan.logpriors[a] = logprior;
        for (size_t h = 0; h < nh; h++) {                                 // :2393-2408
            bool ok = filtered[h] == 0;
            if (ok) {
                const VarSet s = variantsOf(haps[h]);
                for (VarSet::const_iterator it = s.begin(); ok && it != s.end(); ++it) ok = activeSets[a].count(*it) != 0;
            }
            plan.compat[a * nh + h] = ok ? 1 : 0;
        }
    }
    plan.logliks.assign(nav, 0.0);
    plan.freqs.assign(nav * nh, 0.0);
}

void pooledRunEM(const std::vector<PooledPlan *> &plans, const std::vector<const PooledWindow *> &wins, const PooledParameters &pp,
                 bool hostEM, int device, int threads)
{
    const size_t W = plans.size();
    std::vector<int32_t> who(W + 1, 0), wro(W + 1, 0), slotWindow;
    std::vector<int64_t> slotOff(1, 0);
    std::vector<uint8_t> compat;
    std::vector<double> ll;
    for (size_t w = 0; w < W; w++) {
        const size_t nh = wins[w]->nh, nr = wins[w]->nr;
        who[w + 1] = who[w] + int32_t(nh); wro[w + 1] = wro[w] + int32_t(nr);
        ll.insert(ll.end(), wins[w]->ll.begin(), wins[w]->ll.end());
        for (int a = 0; a < plans[w]->nav; a++) { slotWindow.push_back(int32_t(w)); slotOff.push_back(slotOff.back() + int64_t(nh)); }
        compat.insert(compat.end(), plans[w]->compat.begin(), plans[w]->compat.end());
    }
    const size_t N = slotWindow.size();
    std::vector<double> loglik(N + 1), freqs(size_t(slotOff.back()) + 1), ediff(N + 1);
    std::vector<int32_t> iters(N + 1);
    if (N > 0) {
        if (ll.empty()) ll.push_back(0.0);
        if (compat.empty()) compat.push_back(0);
        dd_batch b = dd_batch();
        b.n_windows = int32_t(W); b.win_hap_off = who.data(); b.win_read_off = wro.data();
        dd_pooled_slots s = {int64_t(N), slotWindow.data(), slotOff.data(), compat.data()};
        dd_pooled_result out = {loglik.data(), freqs.data(), iters.data(), ediff.data()};
#ifdef DD_POOLED_EM_STANDALONE                  // a program without the library (tests/pooled_em_check.cpp): the CPU evaluation alone
        (void)device;
        const int rc = hostEM ? dd_pooled_em_host(&b, ll.data(), &s, pp.a0, pp.EMtol, &out, threads) : DD_ERR_NO_DEVICE;
        if (rc != DD_SUCCESS) throw std::runtime_error("pooled EM failed");
#else
        const int rc = hostEM ? dd_pooled_em_host(&b, ll.data(), &s, pp.a0, pp.EMtol, &out, threads)
                              : dd_pooled_em(&b, ll.data(), &s, pp.a0, pp.EMtol, &out, device);
        if (rc != DD_SUCCESS) throw std::runtime_error(std::string(hostEM ? "dd_pooled_em_host: " : "dd_pooled_em: ") + dd_last_error());
#endif
    }
    size_t slot = 0;
    for (size_t w = 0; w < W; w++) {
        const size_t nh = wins[w]->nh;
        for (int a = 0; a < plans[w]->nav; a++, slot++) {
            plans[w]->logliks[size_t(a)] = loglik[slot];
            for (size_t h = 0; h < nh; h++) plans[w]->freqs[size_t(a) * nh + h] = freqs[size_t(slotOff[slot]) + h];
        }
        plans[w]->ready = true;
    }
}

void pooledLines(const std::vector<Haplotype> &haps, const std::vector<Read> &reads, const PooledWindow &win, const PooledPlan &plan,
                 uint32_t candPos, uint32_t leftPos, uint32_t rightPos, OutputData &glfData, int index, const std::string &tid,
                 const AlignedCandidates &candidateVariants, const DiploidParameters &params, const std::string &program, size_t numPools)
{
    const size_t nh = haps.size(), nr = reads.size(), nv = plan.allVariants.size(), nav = size_t(plan.nav);
    std::vector<double> rl(nh * nr);
    for (size_t h = 0; h < nh; h++)
        for (size_t r = 0; r < nr; r++) rl[r * nh + h] = win.ll[h * nr + r];
    int numUnmappedRealigned = 0;                                        // :2125-2139
    for (size_t r = 0; r < nr; r++) {
        bool offAll = true;
        for (size_t h = 0; h < nh; h++) if (!win.offHap[h * nr + r]) offAll = false;
        if (!offAll && reads[r].isUnmapped()) numUnmappedRealigned++;
    }
    // :2541-2562
    double logz = -HUGE_VAL;
    for (size_t a = 0; a < nav; a++) logz = addLogs(logz, plan.logliks[a] + plan.logpriors[a]);
    std::vector<double> hapFreqs(nh, 0.0);
    for (size_t a = 0; a < nav; a++)
        for (size_t h = 0; h < nh; h++) hapFreqs[h] += exp(plan.logliks[a] + plan.logpriors[a] - logz) * plan.freqs[a * nh + h];

    std::vector<std::vector<int> > readsOf(numPools);                    // ascending r, like the reference's std::set<int>
    for (size_t r = 0; r < nr; r++) readsOf[size_t(reads[r].poolID)].push_back(int(r));
    const double log5 = log(0.5);
    std::vector<double> prior(nh * nh, 0.0);
    for (size_t v = 0; v < nv; v++) {
        const PAV &pav = plan.allVariants[v];
        double logp = -HUGE_VAL, freq = 0.0;
        for (size_t a = 0; a < nav; a++) if (plan.active[a * nv + v]) logp = addLogs(logp, plan.logliks[a] + plan.logpriors[a]);
        for (size_t h = 0; h < nh; h++) if (plan.hapHasVar[h * nv + v]) freq += hapFreqs[h];
        logp -= logz;
        const bool doGLF = params.outputGLF && candidateOf(pav.second, leftPos, candidateVariants) != NULL;
        if (doGLF) {
            // haplotypes that differ in this variant only fall into one marginal state; its frequency is the pair prior's term (:2614-2662)
            std::vector<int> weight(nv, 0);
            int s = 1;
            for (size_t y = 0; y < nv; y++) if (y != v) { weight[y] = s; s *= 2; }
            std::map<int, int> stateOf;
            std::vector<int> otn(nh);
            for (size_t h = 0; h < nh; h++) {
                int key = 0;
                for (size_t y = 0; y < nv; y++) key += weight[y] * plan.hapHasVar[h * nv + y];
                std::map<int, int>::const_iterator it = stateOf.find(key);
                if (it != stateOf.end()) otn[h] = it->second;
                else { const int fresh = int(stateOf.size()); stateOf[key] = fresh; otn[h] = fresh; }
            }
            std::vector<double> marFreqs(stateOf.size(), 0.0);
            for (size_t h = 0; h < nh; h++) marFreqs[size_t(otn[h])] += hapFreqs[h];
            for (size_t m = 0; m < marFreqs.size(); m++) marFreqs[m] = marFreqs[m] < 1e-16 ? -50 : log(marFreqs[m]);
            for (size_t h1 = 0; h1 < nh; h1++)
                for (size_t h2 = h1; h2 < nh; h2++) prior[h1 * nh + h2] = marFreqs[size_t(otn[h1])] + marFreqs[size_t(otn[h2])];
        }
        const bool indel = pav.second.isIndel(), snp = pav.second.isSNP();
        std::map<PAV, VariantCoverage>::const_iterator cov = win.varCoverage.find(pav);
        for (size_t b = 0; b < numPools; b++) {
            double msq = 0.0;
            int nf = 0, nrev = 0;
            double lik[3] = {0.0, 0.0, 0.0};
            const std::vector<int> &mine = readsOf[b];
            if (!mine.empty()) {
                if (doGLF) {
                    for (int i = 0; i < 3; i++) lik[i] = -HUGE_VAL;
                    for (size_t h1 = 0; h1 < nh; h1++)
                        for (size_t h2 = h1; h2 < nh; h2++) {
                            const int genotype = plan.hapHasVar[h1 * nv + v] + plan.hapHasVar[h2 * nv + v];
                            double ll = prior[h1 * nh + h2];                        // prior + t_1 + t_2 + ... (:2687-2690)
                            for (size_t k = 0; k < mine.size(); k++) { const size_t r = size_t(mine[k]); ll += log5 + addLogs(rl[r * nh + h1], rl[r * nh + h2]); }
                            lik[genotype] = addLogs(lik[genotype], ll);
                        }
                }
                for (size_t k = 0; k < mine.size(); k++) {
                    const size_t r = size_t(mine[k]);
                    double ml = -HUGE_VAL;
                    for (size_t h = 0; h < nh; h++) if (rl[r * nh + h] >= ml) ml = rl[r * nh + h];
                    bool onReverse = false, onForward = false;
                    for (size_t h = 0; h < nh; h++) {
                        if (!(rl[r * nh + h] >= ml - 1e-7)) continue;               // the most likely haplotypes of the read (:2708-2712)
                        if (plan.hapHasVar[h * nv + v] && (indel || snp) && win.covered(h, r, pav.first, snp)) { if (reads[r].onReverseStrand) onReverse = true; else onForward = true; }
                    }
                    const double mq = -10 * log10(1.0 - reads[r].mapQual);
                    msq += mq * mq;
                    if (onForward) nf++;
                    if (onReverse) nrev++;
                }
                msq = sqrt(msq / double(mine.size()));
            }
            if (!doGLF) continue;
            OutputData::Line line(glfData);
            line.set("msg", "ok").set("index", index).set("tid", tid).set("analysis_type", program).set("indidx", (unsigned long)b);
            line.set("was_candidate_in_window", 1).set("lpos", leftPos).set("rpos", rightPos).set("center_position", candPos);
            line.set("realigned_position", unsigned(pav.first) + leftPos).set("post_prob_variant", exp(logp)).set("est_freq", freq).set("logZ", logz);
            line.set("nref_all", pav.second.getString()).set("num_reads", (unsigned long)mine.size()).set("msq", msq);
            line.set("num_cover_forward", nf).set("num_cover_reverse", nrev).set("num_unmapped_realigned", numUnmappedRealigned);
            line.set("var_coverage_forward", cov == win.varCoverage.end() ? 0 : cov->second.nf);
            line.set("var_coverage_reverse", cov == win.varCoverage.end() ? 0 : cov->second.nr);
            if (b == 0) {                                                           // the haplotypes with their frequencies (:2774-2797)
                std::string text;
                bool firstHap = true;
                for (size_t h = 0; h < nh; h++) {
                    if (!(hapFreqs[h] > 1.0 / double(2 * nr))) continue;
                    if (!firstHap) text += ";";
                    firstHap = false;
                    int nvars = 0;
                    for (VarIt it = haps[h].indels.begin(); it != haps[h].indels.end(); ++it) {
                        if (it->second.getString() == "*REF") continue;
                        if (nvars++) text += ",";
                        text += std::to_string(leftPos + unsigned(it->first)) + "," + it->second.getString();
                    }
                    if (nvars == 0) text += "REF";
                    text += ":" + g6(hapFreqs[h]);
                }
                line.set("hapfreqs", text);
            }
            line.set("glf", "0/0:" + g6(lik[0]) + ";0/1:" + g6(lik[1]) + ";1/1:" + g6(lik[2]));
            glfData.output(line);
        }
    }
}

} // namespace dindel
