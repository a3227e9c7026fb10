"""The hysteresis step of the two sweeps as compare-to-EXEC + predicated moves (hmm_kernel.hip take_if_above, the PRED_STEP builds:
whole-wavefront K <= 2 at D = 6), on the inputs where "take iff val > best + EPS" decides something.

  ties      five windows of 117 .. 123-bp haplotypes (the folded, the mirrored and the one-lane form of RO) that hold a homopolymer run and a
            tandem repeat, 12 reads of 30 .. 58 bp lying inside the run / the repeat: later candidates EQUAL the incumbent and stay untaken
  eps       the `tie` parameter set (tests/_param_cases.py: emissions 2e-10 apart) on its two windows with the 136 .. 146-bp read ladder:
            candidates that beat the incumbent by 2e-10, just above EPS, and exact ties beside them, in one launch
  minus_inf haplotypes of 3 .. 8 bp (numS <= 10: shorter than D + 2, most lanes hold no state) under reads that hang over the right end, at
            maxLengthDel 2 and 5: candidates switched off with -inf against an incumbent of -inf
  held      the repeat windows of tests/_path_scenarios.py (ties_windows, 120 bp: a read longer than the repeat, so that an indel has to sit
            somewhere inside it): a later candidate LARGER than the incumbent by rounding, inside (0, EPS], stays untaken
  later items: the ties batch tiled, so that a workgroup takes a second and a third item

Every case runs on every PRED_STEP build its haplotype lengths can reach (the launch log says which kernel ran) and every dd_result field is
compared bit for bit with the oracle.  No half-wave build has the step, so there is no narrowed-EXEC case.

What the chains of those inputs hold is shown on the CPU first (test_hysteresis_decides_on_cpu): a restatement of the oracle's two sweeps
(oracle/dd_oracle.c pass_two_inc / pass_two_dec and the join; its log-likelihood must equal the oracle's bit for bit, which ties it to the
oracle's back-pointers) records every "> best + EPS" step of the chains the kernel runs through take_if_above.  Found there, per batch (the
figures are asserted below): ties — exact ties in a hundred steps and chains whose winner is not the last of their maxima (a `>=` would
move the back-pointer), nothing inside (0, EPS]: reads inside a repeat need no indel; held — steps with a difference inside (0, EPS] and
chains whose winner is not their arg-max at all; eps — exact ties and takes by (EPS, 3 EPS]; no in-chain difference inside (0, EPS] exists
under `tie` (a jump costs 11.5 there, so two candidates of one chain come that close only when they are equal), so that interval is the
held batch's."""
import collections
import math
import os

import numpy as np
import pytest

from dindel_tgi_amd import capi
from dindel_tgi_amd.batch import ReadRec, Window, pack
from tests import _oracle
from tests import _param_cases as pc
from tests import _path_scenarios as ps

EPS = 1e-10
NEG = -math.inf
KEYS = ("DD_DYNAMIC", "DD_FORCE_GBT", "DD_NO_HALF", "DD_NO_FOLD")
RULE = {"dd_hmm_kernel<%d, 6, %s, %s, 0, 1>" % (K, g, f) for K, g, f in
        ((1, "false", "false"), (1, "true", "false"), (1, "false", "true"), (2, "false", "false"), (2, "true", "false"), (2, "false", "true"), (2, "true", "true"))}
# the environments that reach them: the FOLD build (LDS back-pointers), its scratch twin, the one-lane blocks of both
ENVS_K2 = (({"DD_FORCE_GBT": "0"}, "dd_hmm_kernel<2, 6, false, true, 0, 1>"), ({"DD_FORCE_GBT": "1"}, "dd_hmm_kernel<2, 6, true, true, 0, 1>"),
           ({"DD_NO_FOLD": "1", "DD_FORCE_GBT": "0"}, "dd_hmm_kernel<2, 6, false, false, 0, 1>"), ({"DD_NO_FOLD": "1", "DD_FORCE_GBT": "1"}, "dd_hmm_kernel<2, 6, true, false, 0, 1>"))
ENVS_K1 = (({"DD_NO_HALF": "1", "DD_FORCE_GBT": "0"}, "dd_hmm_kernel<1, 6, false, true, 0, 1>"), ({"DD_NO_HALF": "1", "DD_FORCE_GBT": "1"}, "dd_hmm_kernel<1, 6, true, false, 0, 1>"),
           ({"DD_NO_HALF": "1", "DD_NO_FOLD": "1", "DD_FORCE_GBT": "0"}, "dd_hmm_kernel<1, 6, false, false, 0, 1>"))
LAUNCHED = set()


# ---------------------------------------------------------------- the batches (built once, shared, never modified)
TIE_LENGTHS = (117, 118, 120, 121, 123)
TIE_UNITS = ("AC", "CAG", "AC", "GT", "CAG")
HOM_LENS, REP_LENS = (30, 33, 36, 39), (30, 34, 38, 42, 46, 50, 54, 58)


def ties_windows():
    rng = np.random.default_rng(1117)
    ws = []
    for n, unit in zip(TIE_LENGTHS, TIE_UNITS):
        hom, rep = "T" * 40, unit * (60 // len(unit))
        left = ps.rnd(rng, 6, "ACG")
        at_hom, at_rep = len(left), len(left) + len(hom) + 3
        hap = left + hom + ps.rnd(rng, 3, "ACG") + rep
        hap += ps.rnd(rng, n - len(hap))
        # the same length with one repeat unit / one base of the run taken out and random bases at the right end, where RO sits
        haps = [hap, hap[:at_rep] + hap[at_rep + len(unit):] + ps.rnd(rng, len(unit)), hap[:at_hom] + hap[at_hom + 1:] + ps.rnd(rng, 1), ps.rnd(rng, n)]
        assert all(len(h) == n for h in haps)
        reads = [ReadRec("T" * k, [ps.Q30] * k, ps.MQ, ps.HAP_START + at_hom + i) for i, k in enumerate(HOM_LENS)]
        reads += [ReadRec((rep * 2)[i % 2:i % 2 + k], [ps.Q30] * k, ps.MQ, ps.HAP_START + at_rep + i % 2) for i, k in enumerate(REP_LENS)]
        assert len(reads) == 12 and all(30 <= len(r.seq) <= 60 and (r.seq in hom or r.seq in rep) for r in reads)
        hv, hf = ps.variants(haps)
        ws.append(Window(ps.HAP_START, haps, reads, hap_vars=hv, hap_var_flanks=hf))
    return ws


def minus_inf_windows(mld):
    rng = np.random.default_rng(338 + mld)
    ws = []
    for n in range(3, 9):
        hap = ps.rnd(rng, n)
        haps = [hap, hap[:-1] + ("A" if hap[-1] != "A" else "C")]
        reads = []
        for i, L in enumerate((12, 20, 28, 36)):
            s = i % n                                                    # starts inside the haplotype, hangs over its right end
            reads.append(ReadRec(hap[s:] + ps.rnd(rng, L - (n - s)), [ps.Q30] * L, ps.MQ, ps.HAP_START + s))
        reads.append(ReadRec(ps.rnd(rng, 5) + hap + ps.rnd(rng, 9), [ps.Q20] * (n + 14), ps.MQ, ps.HAP_START - 5))      # over both ends
        reads.append(ReadRec(hap[-1] + ps.rnd(rng, 15), [ps.Q30] * 16, 0.9, ps.HAP_START + n - 1))                      # its first base on the last state
        hv, hf = ps.variants(haps)
        ws.append(Window(ps.HAP_START, haps, reads, hap_vars=hv, hap_var_flanks=hf))
    return ws


_CACHE = {}


def case(name):
    """-> (batch, parameters, oracle results)"""
    if name not in _CACHE:
        if name == "ties":
            pb, p = pack(ties_windows()), ps.params_for(5, 0)
        elif name == "ties-tiled":
            pb, p = pack(ties_windows() * 40), ps.params_for(5, 0)
        elif name == "held":
            pb, p = pack(ps.ties_windows(np.random.default_rng(5), 120, 50, 5)), ps.params_for(5, 0)
        elif name.startswith("eps"):                                     # eps-120: K = 2, eps-60: K = 1
            pb, p = pc.batch_for(int(name[4:]), 5), pc.params_for("tie", 5)
        else:                                                            # minus_inf-2, minus_inf-5
            mld = int(name.split("-")[1])
            pb, p = pack(minus_inf_windows(mld)), ps.params_for(mld, 0)
        _CACHE[name] = (pb, p, _oracle.batch(p, pb, nthreads=16))
    return _CACHE[name]


# ---------------------------------------------------------------- the oracle's sweeps once more, with a recorder on the hysteresis steps
def hp_error(n):
    hp = (2.9e-5, 2.9e-5, 2.9e-5, 2.9e-5, 4.3e-5, 1.1e-4, 2.4e-4, 5.7e-4, 1.0e-3, 1.4e-3)
    pbe = (hp[max(n, 1) - 1] if n <= 10 else hp[9] + 4.3e-4 * float(n - 10)) * float(n)
    return min(pbe, 0.99)


class Recorder:
    def __init__(self):
        self.n = collections.Counter()

    def step(self, best, val, taken):
        self.n["steps"] += 1
        if val == NEG and best == NEG:
            self.n["inf_inf"] += 1
        elif val == best:
            self.n["exact_tie"] += 1
        elif val > best and not taken:
            self.n["held_within_eps"] += 1
        elif taken and best != NEG and val - best <= 3 * EPS:
            self.n["taken_just_above"] += 1

    def chain(self, vals, winner):
        m = max(vals)
        self.n["chains"] += 1
        self.n["winner_not_argmax"] += vals[winner] < m
        self.n["winner_not_last_max"] += m != NEG and len(vals) - 1 - vals[::-1].index(m) != winner


def scan(vals, rec=None):
    """the reference's scan over candidates of ascending index: take iff > best + EPS"""
    best, w = NEG, 0
    for i, v in enumerate(vals):
        taken = v > best + EPS
        if rec is not None and i > 0:
            rec.step(best, v, taken)
        if taken:
            best, w = v, i
    if rec is not None:
        rec.chain(vals, w)
    return best


def either(best, v):
    """updateMax towards a smaller index: either branch"""
    return v if v > best + EPS or (best <= v <= best + 1e-5) else best


def pair_ll(hap, read, qual, map_qual, read_start, hap_start, P, rec):
    """log-likelihood of a mapped, unpaired read as oracle/dd_oracle.c pair_impl computes it; rec sees the chains of the right->middle pass
    (jump candidates y = 1 .. maxLengthDel + 1, then the insertion edge) and the insertion-edge step of the left->middle pass"""
    Hs, L = len(hap), len(read)
    assert P.maxLengthDel <= Hs and L >= 1 and 0.0 < map_qual < 1.0
    hap_end, read_end = hap_start + Hs, read_start + L - 1
    if read_start > hap_end or read_end < hap_start:
        bMid = L // 2
    else:
        ol_s, ol_e = max(hap_start, read_start), min(hap_end, read_end)
        bMid = (ol_e - ol_s) // 2 + ol_s - read_start
    bMid = min(max(bMid, 0), L - 1)
    numS, RO = Hs + 2, Hs + 1
    T = 2 * numS
    lLL, lFL = math.log(1.0 - P.pFirstgLO), math.log(P.pFirstgLO)
    numT, II = P.maxLengthDel + 2, -.5
    NI = math.log(1.0 - math.exp(II))
    IN, NN = math.log(P.pError), math.log(1 - P.pError)
    lpe, lpne = [math.log(1e-5)] * numS, [math.log(1 - 1e-5)] * numS
    run, perr = 1, hp_error(1)
    lpe[1], lpne[1] = math.log(perr), math.log(1.0 - perr)
    for b in range(1, Hs):
        if hap[b] == hap[b - 1]:
            run += 1
        else:
            perr = hp_error(run)
            lpe[b], lpne[b] = math.log(perr), math.log(1.0 - perr)
            run = 1
    perr = hp_error(run)
    lpe[Hs - 1], lpne[Hs - 1] = math.log(perr), math.log(1.0 - perr)
    obs = []
    for b in range(L):
        pr = qual[b] * (1.0 - P.pMut)
        eq, uq = math.log(.25 + .75 * pr), math.log(.75 + 1e-10 - .75 * pr)
        o = [eq] * T
        for y in range(Hs):
            if not (hap[y] == "N" or hap[y] == read[b]):
                o[y + 1] = uq
        obs.append(o)

    def dec(a1, o1):
        a = [NEG] * T
        a[RO], ro_i = o1[RO] + a1[RO] + lLL + NN, RO
        for v, i in ((o1[Hs] + a1[Hs] + lFL + NN, Hs), (o1[numS + RO] + a1[numS + RO] + lLL + lpe[RO], numS + RO),
                     (o1[numS + Hs] + a1[numS + Hs] + lFL + lpe[Hs], numS + Hs)):
            if v > a[RO] + EPS or (a[RO] <= v <= a[RO] + 1e-5 and ro_i > i):
                a[RO], ro_i = v, i
        for x in range(1, Hs + 1):
            best, bi = NEG, -1
            for y in range(1, numT):
                nx = max(x - y, 0)
                v = o1[nx] + (lpne[x] if y == 1 else lpe[x] + float(y - 1) * II) + a1[nx] + lpne[x]
                if v > best + EPS or (best <= v <= best + 1e-5 and bi > nx):
                    best, bi = v, nx
            v = o1[numS + x - 1] + a1[numS + x - 1] + lpe[x]
            taken = v > best + EPS
            rec.step(best, v, taken)
            a[x] = v if taken else best
        a[0] = o1[0] + a1[0] + NN
        for x in range(0, Hs + 2):
            a[numS + x] = o1[numS + x] + a1[numS + x] + II
        for x in range(1, Hs + 2):
            a[numS + x] = either(a[numS + x], o1[x] + a1[x] + NI)
        return a

    def inc(b1, o1):
        be = [NEG] * T
        be[0] = scan([o1[0] + b1[0] + lLL + NN, o1[1] + b1[1] + lFL + NN, o1[numS] + b1[numS] + lpe[1]])
        for x in range(1, Hs + 1):
            vals = []
            for y in range(1, numT):
                nx = x + y if x + y <= Hs else RO
                lp = lpne[nx] if y == 1 else lpe[nx] + float(y - 1) * II
                vals.append(lp + lpne[nx] + b1[nx] + o1[nx])
            vals.append(o1[numS + x] + b1[numS + x] + lpe[x + 1])
            be[x] = scan(vals, rec)
        be[RO] = scan([o1[RO] + b1[RO] + lpne[RO], o1[numS + RO] + b1[numS + RO]])
        for x in range(0, Hs + 2):
            nx = min(x + 1, RO) if x else 0
            be[numS + x] = either(o1[numS + x] + b1[numS + x] + II, o1[nx] + b1[nx] + NI)
        return be

    alpha, beta = [0.0] * T, [0.0] * T
    for b in range(1, bMid + 1):
        alpha = dec(alpha, obs[b - 1])
    for b in range(L - 1, bMid, -1):
        beta = inc(beta, obs[b])
    mq = 1.0 - map_qual
    if -10.0 * math.log10(mq) > P.mapQualThreshold:
        mq = math.pow(10.0, -P.mapQualThreshold / 10.0)
    ll = NEG
    for x in range(T):
        i, s = divmod(x, numS)
        lpi = IN if i == 1 else math.log(1.0 - math.exp(IN))
        prior = math.log(mq) + lpi + 0.0 if s == 0 else -100.0 if s == RO else 0.0 + math.log(1.0 - mq) + lpi
        v = alpha[x] + obs[bMid][x] + beta[x] + prior
        if v > ll + EPS:
            ll = v
    return ll


def chains_of(name, pairs):
    """The recorder's counts over the given (window, haplotype, read) pairs of a case; the restatement's log-likelihood equals the oracle's."""
    pb, p, want = case(name)
    a = pb.a
    rec = Recorder()
    for w, h, r in pairs:
        g, q = int(a["win_hap_off"][w]) + h, int(a["win_read_off"][w]) + r
        assert a["read_flags"][q] == 0
        hap = bytes(a["hap_seq"][a["hap_seq_off"][g]:a["hap_seq_off"][g + 1]]).decode()
        s0, s1 = int(a["read_seq_off"][q]), int(a["read_seq_off"][q + 1])
        ll = pair_ll(hap, bytes(a["read_seq"][s0:s1]).decode(), [float(a["qual_table"][i]) for i in a["read_qidx"][s0:s1]],
                     float(a["mapq_table"][a["read_mqidx"][q]]), int(a["read_start"][q]), int(a["win_hap_start"][w]), p, rec)
        assert ll == want["ll"][pc.pair_of(pb, w, h, r)], (name, w, h, r, ll, want["ll"][pc.pair_of(pb, w, h, r)])
    return rec.n


def test_hysteresis_decides_on_cpu():
    n = chains_of("ties", [(w, h, r) for w in range(len(TIE_LENGTHS)) for h, r in ((0, 1), (0, 7), (1, 10), (2, 3))])
    print("ties:", dict(n))
    assert n["exact_tie"] >= 100 and n["winner_not_last_max"] >= 2, dict(n)
    n = chains_of("held", [(w, h, 3) for w in range(2) for h in range(2)])              # the read longer than the repeat
    print("held:", dict(n))
    assert n["held_within_eps"] >= 4 and n["winner_not_argmax"] >= 1 and n["exact_tie"] >= 20, dict(n)
    # `tie`: the second window's ordinary 100-bp read inside the haplotype, on the repeat haplotype and its shorter copy, and two rungs of the ladder
    n = chains_of("eps-120", [(1, 0, pc.ROLE[(100, "inside")] - pc.ORDINARY0 + 4 + pc.N_LADDER), (1, 1, pc.ROLE[(100, "inside")] - pc.ORDINARY0 + 4 + pc.N_LADDER),
                              (0, 0, pc.LADDER[6]), (0, 0, pc.LADDER[7])])
    print("eps:", dict(n))
    assert n["taken_just_above"] >= 10 and n["exact_tie"] >= 5 and n["winner_not_last_max"] >= 5, dict(n)
    # minus_inf: what the kernel adds to the oracle's chains is arithmetic — a D = 6 build forms y = 2 .. 6 for every position of every lane: positions
    # past the haplotype's last state have no source state at all (every candidate -inf against an incumbent of -inf), and y > maxLengthDel + 1
    # is switched off everywhere
    for mld in (2, 5):
        pb, p, want = case("minus_inf-%d" % mld)
        lens = np.diff(pb.a["hap_seq_off"])
        assert lens.min() == 3 and lens.max() == 8 and (lens <= 6 + 2).all() and (lens + 2 < 64).all()
        assert (mld + 1 < 6) == (mld == 2)
        ok = want["status"][:pb.n_pairs] == capi.DD_PAIR_OK
        assert ok.any() and (ok.all() == (mld == 2))                    # 3- and 4-bp haplotypes are a hapSize error at maxLengthDel 5
        assert int((want["hpos"][:pb.hpos_len] == capi.DD_HPOS_RO).sum()) > 0      # reads do run off the right end


# ---------------------------------------------------------------- on the device
pytest_gpu = pytest.mark.gpu


@pytest.fixture()
def clean_env():
    saved = {k: os.environ.pop(k, None) for k in KEYS}
    yield
    for k in KEYS:
        os.environ.pop(k, None)
        if saved[k] is not None:
            os.environ[k] = saved[k]


def run_and_compare(lib, name, env, kernel, every_field=True):
    from tests.test_gpu_fold_mirrored_ro import assert_every_field_equal
    from tests.test_gpu_parity import assert_same, run_host_api
    pb, p, want = case(name)
    for k in KEYS:
        os.environ.pop(k, None)
    os.environ.update(env)
    got = run_host_api(lib, p, pb)
    log = capi.launch_log()
    names = {ps.kernel_name(l) for l in log}
    assert names == {kernel}, (name, env, names)
    assert kernel in RULE
    LAUNCHED.add(kernel)
    what = "%s on %s (%r)" % (name, kernel, env)
    d = ps.first_difference(got, want, pb, {})
    assert d is None, (what, d, got[d[0]][d[1]], want[d[0]][d[1]])
    assert_same(got, want, pb)
    if every_field:
        assert_every_field_equal(got, want, pb, what)
    return log


K2 = [pytest.param(e, k, id=k[14:-7].replace(", ", "-")) for e, k in ENVS_K2]
K1 = [pytest.param(e, k, id=k[14:-7].replace(", ", "-")) for e, k in ENVS_K1]


@pytest_gpu
@pytest.mark.parametrize("env,kernel", K2)
def test_exact_ties(lib, clean_env, env, kernel):
    run_and_compare(lib, "ties", env, kernel)


@pytest_gpu
@pytest.mark.parametrize("env,kernel", K2)
def test_held_inside_eps(lib, clean_env, env, kernel):
    run_and_compare(lib, "held", env, kernel, every_field=False)      # (ties_windows carries no variants: the variant arrays are empty)


@pytest_gpu
@pytest.mark.parametrize("env,kernel", K2 + K1)
def test_inside_and_just_outside_eps(lib, clean_env, env, kernel):
    run_and_compare(lib, "eps-120" if kernel in [k for _, k in ENVS_K2] else "eps-60", env, kernel)


@pytest_gpu
@pytest.mark.parametrize("mld", (2, 5))
@pytest.mark.parametrize("env,kernel", K1)
def test_minus_inf_against_minus_inf(lib, clean_env, env, kernel, mld):
    run_and_compare(lib, "minus_inf-%d" % mld, env, kernel, every_field=(mld == 2))   # (maxLengthDel 5: hapSize-error pairs, whose other fields are not written)


@pytest_gpu
@pytest.mark.parametrize("env,kernel", [({"DD_DYNAMIC": "1", "DD_FORCE_GBT": "0"}, "dd_hmm_kernel<2, 6, false, true, 0, 1>"),
                                        ({"DD_FORCE_GBT": "1"}, "dd_hmm_kernel<2, 6, true, true, 0, 1>"),
                                        ({"DD_NO_FOLD": "1", "DD_DYNAMIC": "1", "DD_FORCE_GBT": "0"}, "dd_hmm_kernel<2, 6, false, false, 0, 1>")],
                         ids=["lds-item-counter", "scratch-persistent", "lds-item-counter-one-lane-blocks"])
def test_later_items_of_a_workgroup(lib, clean_env, env, kernel):
    log = run_and_compare(lib, "ties-tiled", env, kernel)
    assert max(l["n_haps"] * l["split"] / l["grid"] for l in log) > 2.0, log          # a workgroup takes a second and a third item


@pytest_gpu
def test_every_build_of_the_rule_ran():
    if len(LAUNCHED) < 2:
        pytest.skip("needs the cases above in the same run")
    assert LAUNCHED == RULE, sorted(RULE - LAUNCHED)
