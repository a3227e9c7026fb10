"""Windows for the certified MAP haplotype pair (dd_diploid_pairs_host / dd_diploid_pairs_device), as flat arrays, built once per process:
seeded synthetic windows in the shapes that matter (H = 1 ... 12 and one window of 65 haplotypes; R in 1, 2, 63, 64, 65, 130, 200, 400; ll
continuous in (-120, 0]; 40 % of the haplotypes share 80 % of their column with haplotype 0; continuous priors), then the constructed cases,
each with the state it must get.  host() is the real host function's answer (maxLikelihoodPair's sums and argmax through
ddh_max_likelihood_pair) for every window it can take."""
import ctypes as C
import functools

import numpy as np

from dindel_tgi_amd import capi
from tests import _host

N_FUZZ = 2060                      # more than the kernel's 2,048 workgroups: the batch takes a second window per wavefront
READ_COUNTS = (1, 2, 63, 64, 65, 130, 200, 400)
INF, NAN = np.inf, np.nan
FUZZ = -1                          # expected state of a synthetic window: whatever it is, it must be certified


def max_likelihood_pair(ll, prior):
    """maxLikelihoodPair's sums and argmax (host, glibc) on one window: ll [H, R], prior [H, H] -> ((h1, h2) or None on its throw, V [H, H])."""
    f = _host.load().ddh_max_likelihood_pair
    f.argtypes = [C.c_int, C.c_int, capi.c_f64p, capi.c_f64p, capi.c_i32p, capi.c_f64p]
    f.restype = C.c_int
    H, R = ll.shape
    ll = np.ascontiguousarray(ll, np.float64)
    pr = np.ascontiguousarray(prior, np.float64)
    pair, vals = np.zeros(2, np.int32), np.zeros((H, H))
    rc = f(H, R, ll.ctypes.data_as(capi.c_f64p), pr.ctypes.data_as(capi.c_f64p), pair.ctypes.data_as(capi.c_i32p), vals.ctypes.data_as(capi.c_f64p))
    return (None if rc else (int(pair[0]), int(pair[1]))), vals


def fuzz_window(rng, H, R):
    ll = -120.0 * rng.random((H, R))
    for h in range(1, H):
        if rng.random() < 0.4:
            same = rng.random(R) < 0.8
            ll[h, same] = ll[0, same]
    return ll, -30.0 * rng.random((H, H))


def ulp_apart_window(rng):
    """Two haplotypes whose pairs (0, 0) and (0, 1) the host puts 1 ... 4 ulp apart: prior[0, 1] is nudged in ulp steps until they are."""
    ll = -40.0 * rng.random((2, 10))
    prior = np.array([[-5.0, 0.0], [0.0, -1000.0]])
    _, v = max_likelihood_pair(ll, prior)
    prior[0, 1] = v[0, 0] - v[0, 1]
    for _ in range(4096):
        _, v = max_likelihood_pair(ll, prior)
        d = (v[0, 1] - v[0, 0]) / np.spacing(abs(v[0, 0]))
        if 1 <= d <= 4:
            return ll, prior
        prior[0, 1] = np.nextafter(prior[0, 1], INF if d < 1 else -INF)
    raise AssertionError("no prior puts the two pairs 1 ... 4 ulp apart")


@functools.lru_cache(maxsize=None)
def build():
    """dict(ho, ro [W + 1] int32; po, hh [W + 1] int64; ll, status per pair; prior; expect [W]: the state, or FUZZ; names {w: case})."""
    rng = np.random.default_rng(20261020)
    wins, names = [], {}

    def add(ll, prior, status=None, expect=FUZZ, name=None):
        ll = np.asarray(ll, np.float64)
        if name:
            names[name] = len(wins)
        wins.append((ll, np.asarray(prior, np.float64), np.zeros(ll.shape, np.int32) if status is None else status, expect))

    empty = (np.zeros((0, 0)), np.zeros((0, 0)))
    add(*empty, expect=capi.DD_DIPPAIR_NO_HAPS, name="empty_first")
    for i in range(N_FUZZ):
        H = 65 if i == 7 else int(rng.integers(1, 13))
        add(*fuzz_window(rng, H, READ_COUNTS[i % len(READ_COUNTS)] if i != 7 else 65))
    col = -50.0 * rng.random(30)
    add(np.stack([col, col]), np.full((2, 2), -3.25), expect=capi.DD_DIPPAIR_TIE, name="identical_columns")
    add(*empty, expect=capi.DD_DIPPAIR_NO_HAPS, name="empty_between")
    add(*ulp_apart_window(rng), expect=capi.DD_DIPPAIR_TIE, name="ulp_apart")
    for vname, v in (("nan", NAN), ("ninf", -INF), ("pinf", INF)):
        for where in ("first", "last", "not_best"):
            ll, prior = fuzz_window(rng, 4, 64)
            if where == "not_best":                       # pair (3, 3) is far from the best: its prior says so
                prior[:, 3] = -5000.0
                ll[3, 17] = v
            else:
                ll[int(rng.integers(0, 4)), 0 if where == "first" else 63] = v
            add(ll, prior, expect=capi.DD_DIPPAIR_NONFINITE, name="%s_%s" % (vname, where))
    add(np.full((3, 5), -INF), -rng.random((3, 3)), expect=capi.DD_DIPPAIR_NONFINITE, name="all_ninf")
    ll, prior = fuzz_window(rng, 3, 20)
    prior[0, 2] = NAN
    add(ll, prior, expect=capi.DD_DIPPAIR_NONFINITE, name="nan_prior")
    ll, prior = fuzz_window(rng, 3, 20)
    add(ll, np.full((3, 3), -INF), expect=capi.DD_DIPPAIR_NONFINITE, name="all_priors_ninf")
    ll, prior = fuzz_window(rng, 5, 65)
    st = np.zeros(ll.shape, np.int32)
    st[2, 64] = capi.DD_PAIR_NAN
    add(ll, prior, st, expect=capi.DD_DIPPAIR_NOT_COMPUTED, name="status")
    ll, prior = fuzz_window(rng, 5, 65)
    ll[1, 3] = NAN
    st = np.zeros(ll.shape, np.int32)
    st[4, 0] = capi.DD_PAIR_UNSUPPORTED
    add(ll, prior, st, expect=capi.DD_DIPPAIR_NOT_COMPUTED, name="status_before_nan")
    add(np.zeros((0, 7)), np.zeros((0, 0)), expect=capi.DD_DIPPAIR_NO_HAPS, name="reads_without_haplotypes")
    add(*fuzz_window(rng, 1, 33), expect=capi.DD_DIPPAIR_CERTIFIED, name="one_haplotype")
    add(np.zeros((3, 0)), np.array([[-4.0, -2.5, -9.0], [0.0, -3.0, -2.75], [0.0, 0.0, -8.0]]), expect=capi.DD_DIPPAIR_CERTIFIED, name="no_reads")
    H = capi.DD_DIPPAIR_MAX_HAPS
    add(*fuzz_window(rng, H, 3), expect=capi.DD_DIPPAIR_CERTIFIED, name="most_haplotypes")
    add(*fuzz_window(rng, H + 1, 1), expect=capi.DD_DIPPAIR_TOO_MANY_HAPS, name="too_many_haplotypes")
    add(*empty, expect=capi.DD_DIPPAIR_NO_HAPS, name="empty_last")

    nh = np.array([w[0].shape[0] for w in wins], np.int64)
    nr = np.array([w[0].shape[1] for w in wins], np.int64)
    z = np.zeros(1, np.int64)
    c = dict(ho=np.concatenate([z, np.cumsum(nh)]).astype(np.int32), ro=np.concatenate([z, np.cumsum(nr)]).astype(np.int32),
             po=np.concatenate([z, np.cumsum(nh * nr)]), hh=np.concatenate([z, np.cumsum(nh * nh)]),
             ll=np.concatenate([w[0].reshape(-1) for w in wins]), prior=np.concatenate([w[1].reshape(-1) for w in wins]),
             status=np.concatenate([w[2].reshape(-1) for w in wins]), expect=np.array([w[3] for w in wins], np.int32), names=names,
             nh=nh, nr=nr, n_windows=len(wins))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def window(c, w):
    """Window w of build()'s arrays: (ll [H, R], prior [H, H], status [H, R])."""
    H, R = int(c["nh"][w]), int(c["nr"][w])
    p0, h0 = int(c["po"][w]), int(c["hh"][w])
    return c["ll"][p0:p0 + H * R].reshape(H, R), c["prior"][h0:h0 + H * H].reshape(H, H), c["status"][p0:p0 + H * R].reshape(H, R)


@functools.lru_cache(maxsize=None)
def twin():
    """dd_diploid_pairs_host over build()'s windows as one batch: dict(pair, state, best, gap, margin)."""
    c = build()
    out = capi.diploid_pairs_host(c["ho"], c["ro"], c["ll"], c["prior"], c["status"], nthreads=8)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def host():
    """The host function on every window whose ll, status and prior it can take (all finite, all computed, H > 0):
    {w: ((h1, h2), V [H, H])}."""
    c = build()
    res = {}
    for w in range(c["n_windows"]):
        ll, prior, st = window(c, w)
        if ll.shape[0] == 0 or st.any() or not np.isfinite(ll).all() or not np.isfinite(prior[np.triu_indices(ll.shape[0])]).all():
            continue
        res[w] = max_likelihood_pair(ll, prior)
    return res
