"""The pooled analysis' EM arithmetic on the CPU (csrc/pooled_math.h, dd_pooled_em_host) against exact arithmetic.

The fixtures (tests/golden/pooled_math.json, pooled_em.json) are 50-digit values written by tests/golden/make_pooled_em_fixtures.py.

Function accuracy: the error of pm_exp / pm_log / pm_digamma over the fixed grids, in ulp of max(1, |f|), measured on the CPU:
exp 0.181, log 0.681, digamma 4.038 (the bounds below are these rounded up in the third decimal).  These are deterministic functions of a fixed grid (fp64 operations and literals
only), so the measured maxima are the bounds; all are far inside the 1e-12 relative the project accepts between device and glibc functions.

Host EM against exact EM: equal iteration counts on every case, and the relative deviation of loglik and of every frequency at most
8 x the largest measured on the CPU over the fixture, 8 x 1.11e-14 (the margin is for a libm that differs: the loop itself calls none, only
fma() where the host has no such instruction).
"""
import json
import os
import subprocess
from decimal import Decimal, getcontext

import numpy as np
import pytest

from dindel_tgi_amd import pooled

getcontext().prec = 70
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ULP_BOUND = {"exp": 0.182, "log": 0.682, "digamma": 4.039}       # measured maxima, see the module text
EM_MEASURED = 1.11e-14                                        # largest relative deviation of loglik / freqs measured over pooled_em.json
REL_1E12 = 1e-12


def _ulp_of_max1(v):
    a = max(Decimal(1), abs(v))
    e = a.adjusted()                                  # decimal exponent; the binary one by comparison
    k = int(e * 3.3219280948873626) - 2
    while Decimal(2) ** (k + 1) <= a:
        k += 1
    return Decimal(2) ** (k - 52)


@pytest.mark.parametrize("fn", ["exp", "log", "digamma"])
def test_function_accuracy(lib, fn):
    grid = json.load(open(os.path.join(GOLDEN, "pooled_math.json")))[fn]
    x = np.array([float.fromhex(g[0]) for g in grid])
    got = pooled.math_eval(fn, x)
    worst, worst_rel, at = Decimal(0), Decimal(0), None
    for xi, gi, (_, want) in zip(x, got, grid):
        w = Decimal(want)
        err = abs(Decimal(float(gi)) - w)
        u = err / _ulp_of_max1(w)
        if u > worst:
            worst, at = u, xi
        worst_rel = max(worst_rel, err / max(Decimal(1), abs(w)))
    print("%s: max error %.3f ulp of max(1,|f|) at x=%r, %.3g relative to max(1,|f|), %d points" % (fn, worst, at, worst_rel, len(x)))
    assert worst_rel < REL_1E12                        # beyond this the series is defective, not a bound to adopt
    assert worst <= ULP_BOUND[fn]


def test_exp_edges(lib):
    inf = float("inf")
    got = pooled.math_eval("exp", np.array([-inf, -800.0, -745.0, -708.3964185322642, 0.0]))
    assert got.tolist() == [0.0, 0.0, 0.0, 0.0, 1.0]   # below the normal range: 0, never a denormal
    assert pooled.math_eval("exp", np.array([-708.3964185322641]))[0] >= 2.0 ** -1022
    assert pooled.math_eval("log", np.array([1.0, 0.0, inf])).tolist() == [0.0, -inf, inf]


def test_add_logs(lib):
    inf = float("inf")
    pairs = np.array([[-inf, -3.5], [-3.5, -inf], [-10.0, -10.0], [-5.0, -900.0], [-1e300, -7.0], [-inf, -1e300]])
    got = pooled.math_eval("add_logs", pairs)
    assert got[0] == -3.5 and got[1] == -3.5 and got[3] == -5.0 and got[4] == -7.0 and got[5] == -1e300
    assert abs(got[2] - (-10.0 + np.log(2.0))) < 4e-15


def _run_case(c, nthreads=1):
    rl = np.array(c["rl"], np.float64).reshape(len(c["rl"]), len(c["compat"]))
    nr, nh = rl.shape
    ll = np.ascontiguousarray(rl.T).reshape(-1)       # the likelihood kernels' layout: haplotype-major
    who, wro = np.array([0, nh], np.int32), np.array([0, nr], np.int32)
    slots = pooled.pack_slots(who, [0], [c["compat"]])
    return pooled.em_host(who, wro, ll, slots, a0=c["a0"], tol=c["tol"], nthreads=nthreads)


def test_host_em_against_exact_em(lib):
    cases = json.load(open(os.path.join(GOLDEN, "pooled_em.json")))["cases"]
    assert len(cases) >= 10
    worst = Decimal(0)
    for i, c in enumerate(cases):
        assert c["closest_to_tol"] >= 1e-7            # the generator's guard: no convergence decision fp64 can flip
        got = _run_case(c)
        assert int(got["iters"][0]) == c["iters"], (i, c["kind"])
        dev = [abs(Decimal(float(got["loglik"][0])) / Decimal(c["loglik"]) - 1)]
        dev += [abs(Decimal(float(g)) / Decimal(w) - 1) for g, w in zip(got["freqs"], c["freqs"])]
        print("case %d (%d reads x %d haplotypes, %s): %d iterations, largest relative deviation %.3g" %
              (i, len(c["rl"]), len(c["compat"]), c["kind"], c["iters"], max(dev)))
        worst = max(worst, max(dev))
    print("largest relative deviation over the fixture: %.3g" % worst)
    assert worst <= Decimal(8 * EM_MEASURED)


def test_host_em_threads_and_ragged_batch(lib):
    """Several windows and slots in one call, on one thread and on four: the same bits as one slot at a time."""
    cases = json.load(open(os.path.join(GOLDEN, "pooled_em.json")))["cases"][:6]
    who = np.concatenate([[0], np.cumsum([len(c["compat"]) for c in cases])]).astype(np.int32)
    wro = np.concatenate([[0], np.cumsum([len(c["rl"]) for c in cases])]).astype(np.int32)
    ll = np.concatenate([np.array(c["rl"], np.float64).reshape(len(c["rl"]), -1).T.reshape(-1) for c in cases])
    sw = [0, 1, 1, 2, 3, 4, 5, 5]
    compat = [cases[w]["compat"] if k % 2 == 0 else [1] * len(cases[w]["compat"]) for k, w in enumerate(sw)]
    slots = pooled.pack_slots(who, sw, compat)
    one = pooled.em_host(who, wro, ll, slots, nthreads=1)
    four = pooled.em_host(who, wro, ll, slots, nthreads=4)
    for k in one:
        assert np.array_equal(one[k], four[k]), k
    for k, w in enumerate(sw):
        single = _run_case(dict(cases[w], compat=compat[k], a0=0.001, tol=1e-4))
        o = int(slots["slot_off"][k])
        assert one["loglik"][k] == single["loglik"][0] and one["iters"][k] == single["iters"][0]
        assert np.array_equal(one["freqs"][o:o + len(compat[k])], single["freqs"])


def test_invalid_arguments(lib):
    who, wro = np.array([0, 2], np.int32), np.array([0, 3], np.int32)
    ll = np.full(6, -10.0)
    slots = pooled.pack_slots(who, [0], [[1, 1]])
    with pytest.raises(RuntimeError):
        pooled.em_host(who, wro, ll, slots, a0=0.0)
    bad = dict(slots, slot_window=np.array([1], np.int32))
    with pytest.raises(RuntimeError):
        pooled.em_host(who, wro, ll, bad)
    empty = pooled.pack_slots(who, [], [])
    assert len(pooled.em_host(who, wro, ll, empty)["loglik"]) == 0
    # no reads: two iterations, the prior's frequencies
    got = pooled.em_host(who, np.array([0, 0], np.int32), np.zeros(0), slots)
    assert got["iters"][0] == 2 and got["loglik"][0] == 0.0 and np.array_equal(got["freqs"], [0.5, 0.5])


def test_pooled_em_check_program(tmp_path):
    """tests/pooled_em_check.cpp with pooled_em_host.cpp and host/pooled_em.cpp, g++ alone, under AddressSanitizer and UBSan; run directly."""
    exe = str(tmp_path / "pooled_em_check")
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-O1", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DDD_POOLED_EM_STANDALONE", "-o", exe, os.path.join(ROOT, "tests", "pooled_em_check.cpp"),
                           os.path.join(ROOT, "dindel_tgi_amd", "csrc", "pooled_em_host.cpp"), os.path.join(ROOT, "dindel_tgi_amd", "host", "pooled_em.cpp"),
                           os.path.join(ROOT, "dindel_tgi_amd", "host", "genotype.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().split("\n")[-1] == "pooled_em_check: ok", (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


# ---- sets, priors, lines: host/pooled_em.cpp on a handmade window against the independent restatement tests/_pooled_oracle.py ----
def handmade_window(filtered=()):
    """A reference haplotype, two indel haplotypes, one with a SNP and an indel, and a "=>D" SNP that must be ignored; candidates with and
    without a frequency (and one variant that is no candidate: no line); three pools, the last one without reads."""
    rng = np.random.default_rng(2103)
    haps = [dict(filtered=0, vars={60: "*REF"}),
            dict(filtered=0, vars={60: "-AC"}),
            dict(filtered=0, vars={60: "+GAT", 75: "*REF"}),
            dict(filtered=0, vars={40: "A=>G", 60: "-AC"}),
            dict(filtered=0, vars={60: "*REF", 90: "C=>D"}),
            dict(filtered=0, vars={60: "*REF", 100: "+T"})]
    for h in filtered:
        haps[h]["filtered"] = 1
    nh, nr = len(haps), 46
    reads = [dict(pool=int(r % 5 != 0), reverse=bool(rng.integers(0, 2)), mapq=1.0 - 10 ** (-float(rng.choice([2.0, 4.0, 6.0]))), unmapped=bool(r % 11 == 3))
             for r in range(nr)]
    origin = [int(rng.choice([0, 0, 1, 2, 3])) if reads[r]["pool"] == 0 else int(rng.choice([0, 0, 0, 3])) for r in range(nr)]
    ll = [[float(rng.uniform(-60, -5)) for _ in range(nr)] for _ in range(nh)]
    for r in range(nr):
        base = ll[0][r]
        for h in range(nh):
            ll[h][r] = base - (0.0 if h == origin[r] else float(rng.choice([0.0, 0.4, 9.0, 25.0])))
    off = [[bool(rng.random() < 0.1) for _ in range(nr)] for _ in range(nh)]
    for r in (3, 14):
        for h in range(nh):
            off[h][r] = True
    covered = set()
    for h, hp in enumerate(haps):
        for k, s in hp["vars"].items():
            for r in range(nr):
                if rng.random() < 0.7:
                    covered.add((h, r, k, int(len(s) == 4 and s[1:3] == "=>")))
    cands = [(5060, "-AC", -1.0), (5060, "+GAT", 0.02), (5040, "A=>G", 0.3), (5090, "C=>D", 0.5)]       # 5100 +T is no candidate
    varcov = {(60, "-AC"): (7, 5), (60, "+GAT"): (3, 0), (40, "A=>G"): (2, 2)}
    return dict(index=7, tid="20", left=5000, right=5120, cand_pos=5060, pools=3, cands=cands, haps=haps, reads=reads, ll=ll, off_hap=off,
                covered=covered, varcov=varcov)


def host_lines(w, program, a0=0.001):
    import ctypes as C
    from dindel_tgi_amd import hostlib
    from tests.test_glf_vcf_cpu import GLF_COLUMNS
    from tests import _pooled_oracle as po
    lib = hostlib.load()
    lib.ddh_pooled_window_lines.argtypes = [C.c_char_p, C.c_char_p, C.c_double, C.c_double, C.c_double, C.c_char_p, C.c_int]
    out = C.create_string_buffer(1 << 20)
    n = lib.ddh_pooled_window_lines(po.window_text(w).encode(), program.encode(), a0, 1e-3, 1e-4, out, len(out))
    assert n >= 0, out.value
    return [dict(zip(GLF_COLUMNS, ln.split(" "))) for ln in out.value.decode().split("\n") if ln]


@pytest.mark.parametrize("filtered", [(), (2,), (0, 3)])
@pytest.mark.parametrize("program", ["all", "singlevariant", "priorpersite"])
def test_sets_priors_lines(program, filtered):
    from tests import _pooled_oracle as po
    from tests.test_glf_vcf_cpu import GLF_COLUMNS
    w = handmade_window(filtered)
    got, want = host_lines(w, program), po.window_lines(w, program)
    # one line per (candidate variant, pool) in allVariants x pool order; the D-SNP and the variant that is no candidate have none
    assert [(r["realigned_position"], r["nref_all"], r["indidx"]) for r in got] == \
        [(str(5000 + k), s, str(b)) for k, s in ((40, "A=>G"), (60, "+GAT"), (60, "-AC")) for b in range(3)]
    assert len(got) == len(want)
    for g_row, w_row in zip(got, want):
        for col in GLF_COLUMNS:
            assert g_row[col] == w_row.get(col, "NA"), (program, filtered, col, g_row[col], w_row.get(col, "NA"))
    for r in got:
        if r["indidx"] == "2":                       # the pool without reads still has its line
            assert r["num_reads"] == "0" and r["glf"] == "0/0:0;0/1:0;1/1:0" and r["msq"] == "0"
        assert (r["hapfreqs"] != "NA") == (r["indidx"] == "0")
    assert got[0]["num_unmapped_realigned"] == str(sum(1 for i in range(46) if i % 11 == 3 and i not in (3, 14)))


def test_unknown_bayes_type_ends_the_run(tmp_path):
    """An unknown --bayesType prints "Unknown EM option" and exits with 1 (DInDel.cpp:2287-2288), before any file is opened."""
    drv = os.path.join(ROOT, "dindel_tgi_amd", "host", "dindel_gpu")
    env = dict(os.environ)
    import torch
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([drv, "--bamFile", "none.bam", "--varFile", "none.txt", "--hapFile", "none.txt", "--outputFile", str(tmp_path / "o"), "--doPooled", "--bayesType", "both"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 1 and "Unknown EM option" in r.stderr
    r = subprocess.run([drv, "--bamFile", "none.bam", "--varFile", "none.txt", "--hapFile", "none.txt", "--outputFile", str(tmp_path / "o"), "--doPooled", "--outputRealignedBAM"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 1 and "--doDiploid" in r.stderr
