"""The four likelihood kernels under model parameters away from the two default sets, bit-equal to the oracle under the same parameters.

Every other GPU test runs dd_hmm_kernel, dd_long_kernel, dd_faster_kernel and dd_faster_long_kernel with the constants that
params_cli_defaults() or params_struct_defaults() put into dd_build_tables.  Here the parameter sets of tests/_param_cases.py — emissions
that tie or prefer a mismatch, -inf and extreme transition constants, priors below the RO prior, the base-quality threshold moved, and a
read-length ladder that straddles the -99 bound of dd_hmm_kernel's speculative pass — go through every selectable build of the main kernel
(a compiler fault is per build), the two smallest long builds, and the --faster kernels.  tests/test_param_cases_cpu.py shows
on the oracle that the sets and the batch reach what they are named after.  A failure names the set, the shape, the pair and the kernel."""
import ctypes as C
import functools
import os
import time

import numpy as np
import pytest

from dindel_tgi_amd import capi
from dindel_tgi_amd.batch import alloc_result
from tests import _oracle
from tests import _param_cases as pc
from tests import _path_scenarios as ps
from tests.test_gpu_faster import assert_same_faster, run_faster
from tests.test_gpu_parity import assert_same, run_host_api
from tests.test_gpu_path_matrix import launches_of

pytestmark = pytest.mark.gpu

SETS = list(pc.PARAM_SETS)
# the haplotype-length loop of a (set, maxLengthDel) case in the three parts of tests/test_gpu_path_matrix.py: unsplit, the slowest case
# (2.9 s) came within a few percent of that matrix's slowest (3.1 s), which it must not outlast
PARTS = ((1, 382), (383, 574), (575, 766))
CASES = [(name, mld, part) for name in SETS for mld in pc.MLDS for part in range(len(PARTS))
         if any(PARTS[part][0] <= h <= PARTS[part][1] for h in ps.hap_lengths(mld))]
GBT_MODES = (None, "0", "1")
ENV_KEYS = ("DD_FORCE_GBT", "DD_FAST_GROUPS", "DD_DYNAMIC", "DD_NO_HALF")
LONG_POINTS = [(120, 31, 1), (255, 20, 2)]                       # (haplotype length, maxLengthDel, K): the two smallest rows of LONG_GRID
FASTER_POINTS = [(hl, mld) for hl in ps.FASTER_HAP_LENGTHS[:3] for mld in (5, 11)]
FASTER_LONG_POINT = (120, 31)

BUILDS, LAUNCHED, RAN, WALL = set(), {}, set(), {}


@pytest.fixture(scope="module")
def lib():
    return capi.load()


@pytest.fixture()
def clean_env():
    saved = {k: os.environ.pop(k, None) for k in ENV_KEYS}
    yield
    for k in ENV_KEYS:
        os.environ.pop(k, None)
        if saved[k] is not None:
            os.environ[k] = saved[k]


@functools.lru_cache(maxsize=None)
def batch(hl, mld):
    return pc.batch_for(hl, mld)


@functools.lru_cache(maxsize=None)
def long_batch(hl, mld):
    return pc.long_batch_for(hl, mld)


def where_of(pair, pb, log=None):
    """`pair N (window W, H-bp haplotype x L-bp read), kernel ...` for a failure message."""
    mine, hl, rl = launches_of(pair, log or [], pb)
    w = int(np.searchsorted(pb.win_pair_off, pair, side="right")) - 1
    text = "pair %d (window %d, %d-bp haplotype x %d-bp read)" % (pair, w, hl, rl)
    if log is not None:
        text += ", kernel %s (all launches of the call: %s)" % (" / ".join(ps.kernel_name(l) for l in mine) or "?", ", ".join(ps.kernel_name(l) for l in log))
    return text


def compare(got, want, pb, where, log=None):
    """Bit equality with the oracle in everything assert_same compares and in the hpos of every computed pair."""
    diff = pc.first_difference(got, want, pb)
    if diff is not None:
        key, elem, pair = diff
        raise AssertionError("%s: %s: %s[%d] is %r, the oracle has %r" % (where, where_of(pair, pb, log), key, elem, got[key][elem], want[key][elem]))
    assert_same(got, want, pb)


def compare_faster(got, want, pb, where, kernel):
    try:
        assert_same_faster(got, want, pb)
    except AssertionError as e:
        n = pb.n_pairs
        ok = want["status"][:n] == capi.DD_PAIR_OK
        bad = [int(np.nonzero((got[k][:n] != want[k][:n]) & (ok | (k == "status")))[0][0]) for k in ("status", "ll", "llOn", "llOff", "firstBase", "lastBase", "numMismatch", "numIndels")
               if ((got[k][:n] != want[k][:n]) & (ok | (k == "status"))).any()]
        raise AssertionError("%s: %s%s, kernel %s" % (where, e, "; first differing " + where_of(min(bad), pb) if bad else "", kernel))


def record(log):
    for r in log:
        name = ps.kernel_name(r)
        LAUNCHED[name] = LAUNCHED.get(name, 0) + 1
        BUILDS.add((r["K"], r["D"], r["gbt"], r["pairs_per_wave"]))


@pytest.mark.parametrize("name,mld,part", CASES, ids=["%s-mld%d-hap%d..%d" % ((n, m) + PARTS[p]) for n, m, p in CASES])
def test_main_kernel(lib, clean_env, name, mld, part):
    import torch
    from dindel_tgi_amd.device import DeviceBatch
    t0 = time.time()
    p = pc.params_for(name, mld)
    last = None
    for hl in ps.hap_lengths(mld):
        if not PARTS[part][0] <= hl <= PARTS[part][1]:
            continue
        pb = batch(hl, mld)
        want = _oracle.batch(p, pb, nthreads=16)
        for gbt in GBT_MODES:
            os.environ.pop("DD_FORCE_GBT", None)
            if gbt is not None:
                os.environ["DD_FORCE_GBT"] = gbt
            tag = "set %s, maxLengthDel %d, haplotypes of %d bp, DD_FORCE_GBT %s" % (name, mld, hl, gbt)
            got = run_host_api(lib, p, pb)
            log = capi.launch_log()
            record(log)
            compare(got, want, pb, tag, log)
            if name == "tie":                                     # both sides of the speculative pass's bound computed in this one call
                lad = [pc.pair_of(pb, 0, 0, r) for r in pc.LADDER]
                assert (got["status"][lad] == capi.DD_PAIR_OK).all() and (got["ll"][lad] > -99).any() and (got["ll"][lad] < -99).any(), (tag, got["ll"][lad])
        os.environ.pop("DD_FORCE_GBT", None)
        last = (hl, pb, want)
    # the device-pointer entry at the part's last length, where device.py builds the tables
    hl, pb, want = last
    dev = DeviceBatch(pb, p, "cuda:0")
    assert dev.n_skipped == 0
    dev.launch()
    torch.cuda.synchronize()
    log = capi.launch_log()
    record(log)
    compare(dev.results(), want, pb, "set %s, maxLengthDel %d, haplotypes of %d bp, device-pointer path" % (name, mld, hl), log)
    del dev
    RAN.add((name, mld, part))
    WALL[("main", name, mld, part)] = time.time() - t0
    print("parameter matrix %s mld %d haplotypes %d..%d: %.1f s" % ((name, mld) + PARTS[part] + (WALL[("main", name, mld, part)],)))


def test_matrix_launched_every_build(lib, clean_env):
    """From the launch records of the cases above: every (K, Dt, gbt, G) dd_plan_info can return for MLDS with reads of 1 .. 146 bp (the set
    tests/test_param_cases_cpu.py shows to be planned) was launched — under every parameter set, since every set runs the same shapes."""
    if RAN != set(CASES):
        pytest.skip("needs every case of test_main_kernel in the same run (%d of %d ran)" % (len(RAN), len(CASES)))
    can = pc.selectable(lib)
    names = sorted(LAUNCHED)
    print("parameter matrix: %d distinct kernels launched, %d builds of %d selectable: %s" % (len(names), len(BUILDS), len(can), "; ".join(names)))
    slow = sorted(WALL.items(), key=lambda kv: -kv[1])[:5]
    print("parameter matrix, slowest cases: " + ", ".join("%s %.1f s" % (k, v) for k, v in slow))
    from tests import test_gpu_path_matrix as path_matrix
    if path_matrix.WALL:
        print("path matrix, slowest case of this run: %.1f s" % max(path_matrix.WALL.values()))
    assert len(can) >= 50 and not can - BUILDS, (sorted(can - BUILDS), names)


def run_long(lib, p, pb):
    arrs, res = alloc_result(pb, fill=None)
    b = pb.ctypes_batch()
    rc = lib.dd_compute_likelihoods_ex(C.byref(p), C.byref(b), C.byref(res), 0, capi.DD_OPT_LONG_WINDOWS)
    assert rc == 0, capi.last_error()
    return arrs


def run_faster_long(lib, p, pb):
    arrs, res = alloc_result(pb, fill=None)
    b = pb.ctypes_batch()
    rc = lib.dd_compute_likelihoods_faster_ex(C.byref(p), C.byref(b), C.byref(res), 0, capi.DD_OPT_LONG_WINDOWS_FASTER)
    assert rc == 0, capi.last_error()
    return arrs


@pytest.mark.parametrize("name", SETS)
def test_long_kernel(lib, clean_env, name):
    t0 = time.time()
    for hl, mld, K in LONG_POINTS:
        p = pc.params_for(name, mld)
        pb = long_batch(hl, mld)
        tag = "set %s, dd_long_kernel<%d>, haplotypes of %d bp, maxLengthDel %d" % (name, K, hl, mld)
        got = run_long(lib, p, pb)
        log = capi.long_launch_log()
        assert len(log) == 1 and log[0]["K"] == K and log[0]["pairs"] == pb.n_pairs and log[0]["max_read"] == ps.LONG_FORCE_LEN, (tag, log)
        compare(got, _oracle.batch(p, pb, nthreads=16), pb, tag)
    WALL[("long", name)] = time.time() - t0
    print("parameter matrix %s, long kernel: %.1f s" % (name, WALL[("long", name)]))


@pytest.mark.parametrize("name", SETS)
def test_faster_kernel(lib, clean_env, name):
    t0 = time.time()
    for hl, mld in FASTER_POINTS:
        p = pc.params_for(name, mld)
        pb = batch(hl, mld)
        want = _oracle.batch(p, pb, nthreads=16, faster=True)
        for groups in (None, "1"):
            os.environ.pop("DD_FAST_GROUPS", None)
            if groups is not None:
                os.environ["DD_FAST_GROUPS"] = groups
            got = run_faster(lib, p, pb)
            ll = np.zeros(8, np.int32)
            lib.dd_last_launch(C.byref((C.c_int32 * 8).from_buffer(ll)))
            assert int(ll[0]) == (int(groups) if groups else 4), (name, groups, ll)
            compare_faster(got, want, pb, "set %s, haplotypes of %d bp, maxLengthDel %d, DD_FAST_GROUPS %s" % (name, hl, mld, groups), "dd_faster_kernel")
        os.environ.pop("DD_FAST_GROUPS", None)
    WALL[("faster", name)] = time.time() - t0
    print("parameter matrix %s, faster kernel: %.1f s" % (name, WALL[("faster", name)]))


@pytest.mark.parametrize("name", SETS)
def test_faster_long_kernel(lib, clean_env, name):
    t0 = time.time()
    hl, mld = FASTER_LONG_POINT
    p = pc.params_for(name, mld)
    pb = long_batch(hl, mld)
    got = run_faster_long(lib, p, pb)
    log = capi.faster_long_launch_log()
    tag = "set %s, haplotypes of %d bp, maxLengthDel %d" % (name, hl, mld)
    assert len(log) == 1 and log[0]["pairs"] == pb.n_pairs and log[0]["max_read"] == ps.LONG_FORCE_LEN, (tag, log)
    compare_faster(got, _oracle.batch(p, pb, nthreads=16, faster=True), pb, tag, "dd_faster_long_kernel")
    WALL[("faster_long", name)] = time.time() - t0
    print("parameter matrix %s, faster long kernel: %.1f s" % (name, WALL[("faster_long", name)]))


@pytest.mark.parametrize("faster", [False, True], ids=["main", "faster"])
@pytest.mark.parametrize("name", ["tie", "perror_big"])
def test_engine_non_default_parameters(name, faster):
    """One window through LikelihoodEngine (tests/_host.py): the adapter copies ObservationModelParameters into dd_params field by field
    (compute_likelihoods.cpp to_abi), and has only ever copied the defaults."""
    from dindel_tgi_amd.batch import pack
    from tests import _host
    hl, mld = 126, 5
    p = pc.params_for(name, mld)
    ws = pc.case_windows(hl, mld, np.random.default_rng(pc.seed_of(hl, mld)))[:1]
    pb = pack(ws)
    want = _oracle.batch(p, pb, nthreads=16, faster=faster)
    assert (want["status"][:pb.n_pairs] == capi.DD_PAIR_OK).all()
    res = _host.batch(ws, p, faster=faster)
    assert res["mismatch"] == 0 and not res["windows"][0]["error"], res["windows"][0]["error"]
    got = np.asarray(res["windows"][0]["ll"], np.float64)
    bad = np.nonzero(got != want["ll"][:pb.n_pairs])[0]
    assert got.size == pb.n_pairs and bad.size == 0, ("set %s, %s model: %s" % (name, "--faster" if faster else "main", where_of(int(bad[0]), pb)), got[bad[:4]], want["ll"][bad[:4]])
    assert (got != _oracle.batch(pc.default_params(mld), pb, nthreads=16, faster=faster)["ll"][:pb.n_pairs]).any()       # the set reached the kernel

