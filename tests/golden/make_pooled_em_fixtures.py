"""Writes tests/golden/pooled_math.json and tests/golden/pooled_em.json with mpmath at 50 digits; uses no reference code.

pooled_math.json: fixed grids of x with exp x, log x and digamma x as 50-digit strings (x as C99 hex floats: exact).
pooled_em.json: seeded log-likelihood matrices rl[r][h], compatibility masks, a0 and tol, and the EM loop of the reference
(DInDel.cpp:2412-2543: E-step with addLogs folded over h from -inf, counts, variational M-step with digamma, eNew = sum z (pi + rl),
converged = |eOld - eNew| < tol or iter > 25) evaluated in the reference's order in 50-digit arithmetic.  A case in which
| |eOld - eNew| - tol | falls below 1e-7 at some iteration is rejected: no committed case has a convergence decision fp64 can flip.

    python tests/golden/make_pooled_em_fixtures.py
"""
import json
import os
import random

from mpmath import mp, mpf, exp, log, digamma, nstr

mp.dps = 50
HERE = os.path.dirname(os.path.abspath(__file__))
MARGIN = mpf("1e-7")


def s50(v):
    return nstr(v, 50, strip_zeros=False, min_fixed=-1000000, max_fixed=-1000001)      # always scientific


def math_grids():
    rnd = random.Random(20)
    ex = [-745.0 + i * 745.0 / 298 for i in range(299)] + [-1e-300, -1e-17, -1e-10, -1e-5, -0.3465735902799726, -0.34657359027997264,
                                                              -0.6931471805599453, -708.3964185322641, -708.39, -708.4, -36.7, -37.5]
    ex += [-rnd.random() * 40 for _ in range(100)]
    lg = []
    for k in (-1074, -1060, -1023, -1022, -1021, -100, -2, -1, 0, 1, 2, 100, 1022, 1023):
        for m in (1.0, 1.0 + 2.0 ** -52, 2.0 - 2.0 ** -52, 1.5, 1.4142135623730949, 1.4142135623730951, 1.4142135623730954):
            v = m * 2.0 ** k if k > -1023 else (m * 2.0 ** (k + 60)) * 2.0 ** -60
            if v > 0.0:
                lg.append(v)
    for j in range(1, 53):
        lg += [1.0 + 2.0 ** -j, 1.0 - 2.0 ** -j]
    lg += [1.0 + rnd.random() for _ in range(100)] + [rnd.random() * 10 ** rnd.uniform(-5, 5) for _ in range(60)]
    dg = [0.001, 0.0010000000000000002, 0.002, 0.01, 0.1, 0.5, 1.0, 1.001, 1.46, 1.4616, 1.4616321449683622, 1.4616321449683623,
          1.4616321449683625, 1.4617, 1.47, 2.0, 2.001, 5.5, 9.0, 9.001, 9.999999999999998, 10.0, 10.000000000000002, 10.001, 11.0, 12.5,
          20.0, 64.001, 100.0, 1000.001, 1e4, 12345.678, 1e5]
    dg += [0.001 + rnd.random() * 12 for _ in range(60)] + [10 ** rnd.uniform(1, 5) for _ in range(40)]
    out = {}
    for name, xs, f in (("exp", ex, exp), ("log", lg, log), ("digamma", dg, digamma)):
        xs = sorted(set(float(x) for x in xs))
        out[name] = [[x.hex(), s50(f(mpf(x)))] for x in xs]
    return out


def add_logs(l1, l2):
    if l1 > l2:
        return l1 + log(1 + exp(l2 - l1))
    return l2 + log(1 + exp(l1 - l2))


def exact_em(rl, compat, a0, tol):
    """The reference's loop in its own order; returns (loglik, freqs, iters, smallest | |eOld-eNew| - tol |)."""
    nr, nh = len(rl), len(compat)
    rl = [[mpf(v) for v in row] for row in rl]
    a0, tol = mpf(a0), mpf(tol)
    numah = sum(1 for c in compat if c)
    lpi = [log(mpf(1) / numah) if c else mpf(-100) for c in compat]
    pi = [mpf(0)] * nh
    e_old, it, closest, converged = None, 0, None, False
    while not converged:
        nk = [mpf(0)] * nh
        z = [[mpf(0)] * nh for _ in range(nr)]
        loglik = mpf(0)
        for r in range(nr):
            lognorm = None
            for h in range(nh):
                z[r][h] = lpi[h] + rl[r][h]
                lognorm = z[r][h] if lognorm is None else add_logs(lognorm, z[r][h])      # addLogs(-inf, x) = x
            for h in range(nh):
                z[r][h] = exp(z[r][h] - lognorm)
                nk[h] += z[r][h]
            loglik += lognorm
        ahat = sum((nk[h] + a0 for h in range(nh) if compat[h]), mpf(0))
        dahat = digamma(ahat)
        for h in range(nh):
            if compat[h]:
                lpi[h] = digamma(nk[h] + a0) - dahat
                pi[h] = log((a0 + nk[h]) / (numah * a0 + nr))
            else:
                lpi[h] = pi[h] = mpf(-100)
        e_new = mpf(0)
        for r in range(nr):
            for h in range(nh):
                e_new += z[r][h] * (pi[h] + rl[r][h])
        if e_old is not None:
            d = abs(abs(e_old - e_new) - tol)
            closest = d if closest is None or d < closest else closest
        converged = (e_old is not None and abs(e_old - e_new) < tol) or it > 25
        e_old = e_new
        it += 1
    zs = sum((exp(p) for p in pi), mpf(0))
    return loglik, [exp(p) / zs for p in pi], it, closest


def em_cases():
    rnd = random.Random(411)
    shapes = [  # (reads, haplotypes, mask, a0, tol, kind)
        (1, 1, "all", 0.001, 1e-4, "wide"), (5, 2, "all", 0.001, 1e-4, "close"), (17, 3, "all", 1.0, 1e-4, "close"),
        (64, 3, "alt", 0.001, 1e-4, "close"), (65, 4, "all", 0.001, 1e-4, "wide"), (70, 5, "one", 0.001, 1e-4, "close"),
        (40, 4, "all", 0.001, 1e-4, "mixed"), (33, 2, "all", 1.0, 1e-4, "mixed"), (24, 3, "all", 0.001, 1e-4, "close"),
        (130, 3, "all", 0.001, 1e-4, "mixed"), (12, 5, "alt", 1.0, 1e-4, "wide"), (30, 2, "all", 0.001, 1e-4, "equal")]
    cases = []
    for nr, nh, mask, a0, tol, kind in shapes:
        for attempt in range(20):
            rl = []
            for r in range(nr):
                base = rnd.uniform(-150, -5)
                if kind == "wide":
                    row = [rnd.uniform(-150, -5) for _ in range(nh)]
                elif kind == "close":
                    row = [base + rnd.uniform(-1.5, 1.5) for _ in range(nh)]
                elif kind == "equal":
                    row = [-20.0] * nh
                else:
                    row = [base + (rnd.uniform(-2, 2) if rnd.random() < 0.7 else rnd.uniform(-40, 0)) for _ in range(nh)]
                rl.append(row)
            compat = [1] * nh if mask == "all" else [1 if h % 2 == 0 else 0 for h in range(nh)] if mask == "alt" else [0] * (nh - 1) + [1]
            loglik, freqs, iters, closest = exact_em(rl, compat, a0, tol)
            if closest is None or closest >= MARGIN:
                break
        else:
            raise SystemExit("no admissible case for %r" % ((nr, nh, mask, a0, tol, kind),))
        cases.append({"rl": rl, "compat": compat, "a0": a0, "tol": tol, "kind": kind, "loglik": s50(loglik), "freqs": [s50(f) for f in freqs],
                      "iters": iters, "closest_to_tol": float(closest)})
    return cases


if __name__ == "__main__":
    with open(os.path.join(HERE, "pooled_math.json"), "w") as f:
        json.dump(math_grids(), f, indent=0)
    with open(os.path.join(HERE, "pooled_em.json"), "w") as f:
        json.dump({"cases": em_cases()}, f)
    print("wrote pooled_math.json, pooled_em.json")
