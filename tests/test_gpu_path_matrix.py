"""Every per-pair code path on every HMM kernel build the launch plan can select, bit-equal to the oracle.

tests/test_gpu_persistent_rounds.py runs every build on plain synthetic batches; the per-pair paths (the RO-chain redo pass, the near-tie
join replay, hapSize error, screened windows, the coverage flags, the mate prior, half-wave chunks of more than 256 reads, bMid corners,
N / IUPAC bytes, overhanging reads, full quality tables) each ran on a handful of builds only.  A compiler fault is per build:
here one scenario batch that reaches all of those paths (tests/_path_scenarios.py; tests/test_path_scenarios_cpu.py shows on the oracle
that it does) goes through every lane tiling x D build, at haplotype lengths on both sides of every class bound, in the five launch modes of
test_gpu_persistent_rounds.py and once through the device-pointer entry.  A failure names the kernel, the environment, the scenario family
and the pair."""
import os
import time

import numpy as np
import pytest

from dindel_tgi_amd import capi
from tests import _oracle
from tests import _output_ownership as oo
from tests import _path_scenarios as ps
from tests.test_gpu_parity import assert_same, run_host_api
from tests.test_gpu_persistent_rounds import KEYS, MODES

pytestmark = pytest.mark.gpu

# the class loop of a (maxLengthDel, read length) case in three parts, so that a case stays within a few seconds (the oracle's share grows
# with the haplotype length): haplotypes up to 382 bp, 383 .. 574 bp, 575 .. 766 bp (none at maxLengthDel > 11)
PARTS = ((1, 382), (383, 574), (575, 766))
CASES = [(mld, L, part) for mld, L in ps.GRID for part in range(len(PARTS)) if any(PARTS[part][0] <= h <= PARTS[part][1] for h in ps.hap_lengths(mld))]

LAUNCHED = {}            # kernel name -> launches, over the module
BUILDS = set()           # (K, Dt, gbt, G) launched
CHUNK_ON_HALF = set()    # (K, Dt) of the G = 2 launches that took a chunk window
RAN, WALL = set(), {}


@pytest.fixture(scope="module")
def lib():
    return capi.load()


@pytest.fixture()
def clean_env():
    saved = {k: os.environ.pop(k, None) for k in KEYS}
    yield
    for k in KEYS:
        os.environ.pop(k, None)
        if saved[k] is not None:
            os.environ[k] = saved[k]


def record(log, pb, index):
    for r in log:
        name = ps.kernel_name(r)
        LAUNCHED[name] = LAUNCHED.get(name, 0) + 1
        BUILDS.add((r["K"], r["D"], r["gbt"], r["pairs_per_wave"]))
    if "chunk.window" in index:
        w = int(index["chunk.window"][0])
        h0 = int(pb.a["win_hap_off"][w])
        hl = int(pb.a["hap_seq_off"][h0 + 1] - pb.a["hap_seq_off"][h0])
        cls = int(np.searchsorted(capi.HAP_CLASS_BOUNDS, hl))
        for r in log:                    # the launch of the window's tiling that takes its reads (36 .. 60 bp: never the class beyond 160 bp)
            if r["pairs_per_wave"] == 2 and int(np.searchsorted(capi.HAP_CLASS_BOUNDS, r["max_hap"])) == cls and r["min_read"] == 1 and r["max_read"] >= max(ps.CHUNK_LENS):
                CHUNK_ON_HALF.add((r["K"], r["D"]))


def launches_of(pair, log, pb):
    """The launch records that computed a pair: those of its haplotype's tiling whose read interval holds its read."""
    w = int(np.searchsorted(pb.win_pair_off, pair, side="right")) - 1
    R = int(pb.a["win_read_off"][w + 1] - pb.a["win_read_off"][w])
    h, r = divmod(pair - int(pb.win_pair_off[w]), R)
    g, q = int(pb.a["win_hap_off"][w]) + h, int(pb.a["win_read_off"][w]) + r
    hl, rl = int(pb.a["hap_seq_off"][g + 1] - pb.a["hap_seq_off"][g]), int(pb.a["read_seq_off"][q + 1] - pb.a["read_seq_off"][q])
    cls = int(np.searchsorted(capi.HAP_CLASS_BOUNDS, max(hl, 1)))
    return [l for l in log if int(np.searchsorted(capi.HAP_CLASS_BOUNDS, l["max_hap"])) == cls and l["min_read"] <= rl <= l["max_read"]], hl, rl


def compare(got, want, pb, index, log, where):
    """Bit equality with the oracle (tests/test_gpu_parity.assert_same); a difference is reported with the kernel that computed the first
    differing pair, the launch environment, the pair's scenario family and its index."""
    got, exp = ps.with_screened(got, want, pb, index)
    diff = ps.first_difference(got, exp, pb, index)
    if diff is not None:
        key, elem, pair, family = diff
        mine, hl, rl = launches_of(pair, log, pb)
        raise AssertionError("%s: family %s, pair %d (%d-bp haplotype x %d-bp read): %s[%d] is %r, the oracle has %r; kernel %s; all launches of the call: %s"
                             % (where, family, pair, hl, rl, key, elem, got[key][elem], exp[key][elem],
                                " / ".join(ps.kernel_name(l) for l in mine) or "?", ", ".join(ps.kernel_name(l) for l in log)))
    assert_same(got, exp, pb)


@pytest.mark.parametrize("mld,L,part", CASES, ids=["mld%d-L%d-hap%d..%d" % ((m, l) + PARTS[p]) for m, l, p in CASES])
def test_every_path_on_every_build(lib, clean_env, mld, L, part):
    import torch
    from dindel_tgi_amd.device import DeviceBatch
    t0 = time.time()
    for hl in ps.hap_lengths(mld):
        if not PARTS[part][0] <= hl <= PARTS[part][1]:
            continue
        pb, index = ps.batch_for(hl, L, mld)
        p = ps.params_for(mld, 1)
        want = _oracle.batch(p, pb, nthreads=16)
        own = oo.must_write(pb, want, index)                 # every call below starts from poisoned buffers: what it must write, and nothing else
        for env in MODES:
            for k in KEYS:
                os.environ.pop(k, None)
            os.environ.update(env)
            got = run_host_api(lib, p, pb)
            log = capi.launch_log()
            record(log, pb, index)
            where = "maxLengthDel %d, %d-bp reads, haplotypes of %d bp, environment %r" % (mld, L, hl, env)
            compare(got, want, pb, index, log, where)
            oo.assert_owned(got, want, pb, own, where + "; launches: " + ", ".join(ps.kernel_name(l) for l in log))
        for k in KEYS:
            os.environ.pop(k, None)
        # the device-pointer entry: per-class launches on the caller's stream, dd_screen_windows' flags resident with the batch
        dev = DeviceBatch(pb, p, "cuda:0")
        assert dev.n_skipped == 1
        guarded = oo.GuardedDevice(dev)                      # its result tensors: poison inside 256-byte guards
        dev.launch()
        torch.cuda.synchronize()
        log = capi.launch_log()
        record(log, pb, index)
        where = "maxLengthDel %d, %d-bp reads, haplotypes of %d bp, device-pointer path" % (mld, L, hl)
        res = dev.results()
        compare(res, want, pb, index, log, where)
        oo.assert_owned(res, want, pb, own, where + "; launches: " + ", ".join(ps.kernel_name(l) for l in log))
        guarded.check(where)
        del guarded, dev
        # the same arrays with the mate prior switched off: only the mates window's pairs change (an unpaired read has no prior term)
        p0 = ps.params_for(mld, 0)
        w = int(index["mates.window"][0])
        off = _oracle.batch(p0, pb, first_window=w, n_win=1)
        want0 = {k: v.copy() for k, v in want.items()}
        for k, o in (("hpos", pb.win_hpos_off), ("var_covered", pb.win_varcov_off), ("var_fcov", pb.win_varcov_off), ("onHap", pb.a["win_read_off"])):
            want0[k][int(o[w]):int(o[w + 1])] = off[k][int(o[w]):int(o[w + 1])]
        for k in want0:
            if k not in ("hpos", "var_covered", "var_fcov", "onHap"):
                want0[k][int(pb.win_pair_off[w]):int(pb.win_pair_off[w + 1])] = off[k][int(pb.win_pair_off[w]):int(pb.win_pair_off[w + 1])]
        got = run_host_api(lib, p0, pb)
        log = capi.launch_log()
        compare(got, want0, pb, index, log, "maxLengthDel %d, %d-bp reads, haplotypes of %d bp, mapUnmappedReads 0" % (mld, L, hl))
        oo.assert_owned(got, want0, pb, oo.must_write(pb, want0, index), "maxLengthDel %d, %d-bp reads, haplotypes of %d bp, mapUnmappedReads 0" % (mld, L, hl))
        assert (got["ll"][index["mates.usable"]] != want["ll"][index["mates.usable"]]).any()
    RAN.add((mld, L, part))
    WALL[(mld, L, part)] = time.time() - t0
    print("path matrix mld %d L %d haplotypes %d..%d: %.1f s" % ((mld, L) + PARTS[part] + (WALL[(mld, L, part)],)))


def test_the_matrix_launched_every_selectable_build(lib, clean_env):
    """From the kernel names the cases above collected: every (K, Dt, gbt, G) that dd_plan_info can return under the default environment
    (the sweep of tests/test_path_scenarios_cpu.py) was launched, a FOLD build and the K = 3 two-waves variant ran, and the window with
    more than DD_HALF_CHUNK reads ran on a half-wave build of each of the three half-wave tilings at D = 6, 11 and 12."""
    import ctypes as C
    if RAN != set(CASES):
        pytest.skip("needs every case of test_every_path_on_every_build in the same run (%d of %d ran)" % (len(RAN), len(CASES)))
    out = (C.c_int32 * 10)()
    can = set()
    for mld in range(32):
        p = ps.params_for(mld, 0)
        for hl in sorted({1} | {h for b in capi.HAP_CLASS_BOUNDS for h in (b, b + 1) if h <= capi.DD_MAX_HAP_LEN}):
            for rl in list(range(1, 400)) + list(range(400, 1025, 8)) + [1024]:
                if lib.dd_plan_info(C.byref(p), hl, rl, 256, 50, 100, C.byref(out)) == 0:
                    can.add((out[0], out[1], out[2], out[8]))
    names = sorted(LAUNCHED)
    print("path matrix: %d distinct kernels launched: %s" % (len(names), "; ".join(names)))
    print("path matrix wall time per case: " + ", ".join("%s %.1f s" % (k, v) for k, v in sorted(WALL.items())))
    assert len(can) >= 61 and not can - BUILDS, (sorted(can - BUILDS), names)
    assert any(n.endswith(", true, 0, 1>") for n in names), names                               # FOLD
    assert "dd_hmm_kernel<3, 6, true, false, 2, 1>" in names, names                               # K = 3 scratch build for two waves per SIMD
    assert {(K, D) for K in (1, 3, 5) for D in (6, 11, 12)} <= CHUNK_ON_HALF, (sorted(CHUNK_ON_HALF), names)
