"""The once-per-pair code behind the sweeps of dd_hmm_kernel: the coverage flags and the scalar outputs, which the K <= 2 / D = 6 builds store
one lane per field with the pointers read from the kernel-argument segment (hmm_kernel.hip, LANE_OUT); the other builds store them from lane 0.

Every dd_result field bit-equal to the oracle on batches of at most 4 windows: haplotypes with 0, 1, 3 and 9 variants, reads of 20, 64, 65 and
100 bp (one and two trips of the report loop; one of 170 bp for the redo pass), read counts that are no multiple of the wave count, a
screened-out window, a haplotype shorter than maxLengthDel, a pair that redoes the left->middle pass with RO, launches without some of the
optional arrays, and a persistent grid whose workgroups take a second and third item — on the K = 2 / D = 6 LDS build with and without fold,
its scratch build and a half-wave build (selected the way tests/test_gpu_persistent_rounds.py selects builds)."""
import ctypes as C
import os

import numpy as np
import pytest

from dindel_tgi_amd import capi
from dindel_tgi_amd.batch import ReadRec, Window, alloc_result, pack, phred_to_prob
from tests import _oracle
from tests.test_gpu_parity import assert_same, run_host_api

pytestmark = pytest.mark.gpu

KEYS = ("DD_DYNAMIC", "DD_FORCE_GBT", "DD_NO_HALF", "DD_NO_FOLD", "DD_TARGET_BLOCKS")
# (name, switches, what the launch log must show for at least one launch)
BUILDS = (("lds_fold", {}, lambda l: l["K"] == 2 and not l["gbt"] and l["pairs_per_wave"] == 1),
          ("lds_plain", {"DD_NO_FOLD": "1"}, lambda l: l["K"] == 2 and not l["gbt"] and l["pairs_per_wave"] == 1),
          ("scratch", {"DD_FORCE_GBT": "1"}, lambda l: l["K"] == 2 and l["gbt"] and l["pairs_per_wave"] == 1),
          ("half_wave", {}, lambda l: l["pairs_per_wave"] == 2))
MANY_VARS = 9        # more variants than a haplotype of real data carries: several trips' worth for a one-lane loop, one for the lane-parallel one


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


def _seq(rng, n):
    return "".join(rng.choice(list("ACGT"), n))


def _reads(rng, hap, n, L, q=0.999, mq=0.9999, sub=0.02):
    out = []
    for _ in range(n):
        off = int(rng.integers(-L // 2, max(1, len(hap) - L // 2)))
        s = [hap[i] if 0 <= i < len(hap) else rng.choice(list("ACGT")) for i in range(off, off + L)]
        s = [rng.choice(list("ACGT")) if rng.random() < sub else c for c in s]
        out.append(ReadRec("".join(s), [q] * L, mq, 1000 + off))
    return out


def _variants(rng, hs, n):
    """n variants of a haplotype of hs bases: (start, end) and (left flank, right flank, kind) around the middle, a few at the ends."""
    v, f = [], []
    for i in range(n):
        s = int(rng.integers(8, hs - 12)) if i % 4 else (2 if i % 8 else hs - 4)
        e = s + int(rng.integers(0, 4))
        v.append((s, e))
        f.append((s - 1, e + 1, int(rng.integers(0, 3))))
    return v, f


def _window(rng, hs, lens, reads_per_len, nvars=(0, 1, 3, MANY_VARS), extra_haps=0):
    ref = _seq(rng, hs)
    haps = [ref]
    for h in range(1, len(nvars) + extra_haps):
        p = hs // 2 + int(rng.integers(-8, 8))
        haps.append(ref[:p] + ref[p + 1 + h % 3:] if h % 2 else ref[:p] + _seq(rng, 1 + h % 3) + ref[p:])
    vs, fs = zip(*[_variants(rng, len(h), nvars[i % len(nvars)]) for i, h in enumerate(haps)])
    reads = []
    for L in lens:
        reads += _reads(rng, haps[int(rng.integers(0, len(haps)))], reads_per_len, L)
    return Window(1000, haps, reads, hap_vars=list(vs), hap_var_flanks=list(fs))


def _batch(hs, seed):
    """4 windows: mixed read lengths and variant counts; a hapSize-error haplotype and a pair for the RO redo pass; a window the screen rejects."""
    rng = np.random.default_rng(seed)
    w0 = _window(rng, hs, (20, 64, 65, 100), 5)                          # 20 reads ...
    w0.reads += _reads(rng, w0.haps[1], 3, 100)                           # ... + 3: no multiple of 4 waves, nor of 2 pairs x 4 waves
    w1 = _window(rng, hs - 3, (100, 65), 7)
    w1.haps.append("ACGT")                                                # shorter than maxLengthDel: "hapSize error."
    w1.hap_vars.append([(1, 2)]); w1.hap_var_flanks.append([(0, 3, 1)])
    q2 = float(phred_to_prob([2])[0])                                     # 170 unrelated bases at phred 2 score about -0.65 each: below -99
    w1.reads.append(ReadRec(_seq(rng, 170), [q2] * 170, 0.5, 1000))
    w2 = Window(1000, [_seq(rng, 100), _seq(rng, 800)], _reads(rng, w0.haps[0], 3, 64),   # 800-bp haplotype: outside the kernel limits
                hap_vars=[[], []], hap_var_flanks=[[], []])
    w3 = _window(rng, hs + 2, (64, 20, 100), 3)
    return [w0, w1, w2, w3]


def _want(p, ws, bad):
    """The oracle's results with the screened-out windows marked as the kernels mark them (tests/_path_scenarios.py: status, ll, offHap and
    offHapHMQ of such a pair are defined, its reads are on no haplotype; nothing else of it is written) -> batch, expected arrays, and per
    array the elements the library leaves undefined."""
    from dindel_tgi_amd.batch import pair_slices
    pb = pack(ws)
    pw = pack([w if i not in bad else Window(w.hap_start, w.haps[:1], [], hap_vars=[w.hap_vars[0]], hap_var_flanks=[w.hap_var_flanks[0]]) for i, w in enumerate(ws)])
    part = _oracle.batch(p, pw, nthreads=8)
    want = {k: np.zeros_like(v) for k, v in alloc_result(pb)[0].items()}
    undef = {k: [] for k in want}
    for w in range(len(ws)):
        p0, H, R, h0, SL, _ = pair_slices(pb, w)
        r0 = int(pb.a["win_read_off"][w])
        if w in bad:
            want["status"][p0:p0 + H * R] = capi.DD_PAIR_UNSUPPORTED
            want["offHap"][p0:p0 + H * R] = 1
            want["offHapHMQ"][p0:p0 + H * R] = 1
            for k in want:
                if k == "hpos":
                    undef[k] += list(range(h0, h0 + H * SL))
                elif k not in ("var_covered", "var_fcov", "onHap", "status", "ll", "offHap", "offHapHMQ"):
                    undef[k] += list(range(p0, p0 + H * R))
            continue
        q0, _, _, g0, _, _ = pair_slices(pw, w)
        s0 = int(pw.a["win_read_off"][w])
        v0, v1 = int(pb.win_varcov_off[w]), int(pb.win_varcov_off[w + 1])
        u0 = int(pw.win_varcov_off[w])
        for k in want:
            if k == "hpos":
                want[k][h0:h0 + H * SL] = part[k][g0:g0 + H * SL]
            elif k in ("var_covered", "var_fcov"):
                want[k][v0:v1] = part[k][u0:u0 + v1 - v0]
            elif k == "onHap":
                want[k][r0:r0 + R] = part[k][s0:s0 + R]
            else:
                want[k][p0:p0 + H * R] = part[k][q0:q0 + H * R]
    return pb, want, {k: np.array(v, np.int64) for k, v in undef.items()}


@pytest.fixture(scope="module")
def cases():
    p = capi.params_cli_defaults()
    out = {}
    for name, hs, seed in (("k2", 120, 20261), ("half", 140, 20262)):
        ws = _batch(hs, seed)
        pb, want, undef = _want(p, ws, bad=(2,))
        out[name] = (p, pb, want, undef)
    return out


def _assert_all_fields(got, want, pb, what, undef=None):
    try:
        for k, idx in (undef or {}).items():
            got[k][idx] = want[k][idx]
        assert_same(got, want, pb)
        ok = want["status"][:pb.n_pairs] == capi.DD_PAIR_OK
        for k in ("ll", "llOn", "llOff", "mLogBQ"):                           # bit patterns, not values: -0.0 and NaN payloads included
            assert np.array_equal(got[k][:pb.n_pairs][ok].view(np.uint64), want[k][:pb.n_pairs][ok].view(np.uint64)), k
    except AssertionError as e:
        raise AssertionError("%s, launches %r: %s" % (what, capi.launch_log(), str(e)[:400]))


@pytest.mark.parametrize("build", BUILDS, ids=[b[0] for b in BUILDS])
def test_every_field_on_every_build(lib, clean_env, cases, build):
    name, env, is_it = build
    p, pb, want, undef = cases["half" if name == "half_wave" else "k2"]
    os.environ.update(env)
    got = run_host_api(lib, p, pb)
    assert any(is_it(l) for l in capi.launch_log()), capi.launch_log()
    _assert_all_fields(got, want, pb, name, undef)
    st = want["status"][:pb.n_pairs]
    assert (st == capi.DD_PAIR_HAPSIZE).any() and (st == capi.DD_PAIR_UNSUPPORTED).any()
    assert (want["ll"][:pb.n_pairs][st == capi.DD_PAIR_OK] < -99.0).any()          # the RO redo pass ran
    assert want["var_covered"][:pb.var_cov_len].any() and want["var_fcov"][:pb.var_cov_len].any()   # the flags are not all trivially 0


ABSENT = (("llOn", "mLogBQ", "offHap", "nBQT", "lastBase"), ("llOff", "numIndels", "numMismatch", "nmmBQT", "nMMLeft", "nMMRight", "firstBase", "var_covered"),
          ("var_fcov", "hpos", "llOn", "llOff", "mLogBQ"))


@pytest.mark.parametrize("absent", ABSENT, ids=["a", "b", "c"])
@pytest.mark.parametrize("gbt", ["0", "1"])
def test_optional_arrays_absent(lib, clean_env, cases, absent, gbt):
    """A NULL output pointer masks its lane off: that array is not written, every other one equals the oracle."""
    p, pb, want, undef = cases["k2"]
    os.environ["DD_FORCE_GBT"] = gbt
    arrs, res = alloc_result(pb, fill=None)
    for k in absent:
        arrs[k][...] = 0x55
        setattr(res, k, None)
    b = pb.ctypes_batch()
    assert lib.dd_compute_likelihoods(C.byref(p), C.byref(b), C.byref(res), 0) == 0, capi.last_error()
    for k in absent:
        assert (arrs[k] == 0x55).all(), k
        arrs[k][...] = want[k]
    _assert_all_fields(arrs, want, pb, "without %r" % (absent,), undef)


@pytest.mark.parametrize("gbt", ["0", "1"])
def test_second_and_third_item_of_a_workgroup(lib, clean_env, gbt):
    """More than twice as many items as the persistent grid holds workgroups: what a workgroup keeps per item (offsets, variant count,
    lane constants) is formed again for its second and third haplotype while the wavefronts' buffers are reused."""
    rng = np.random.default_rng(20263)
    p = capi.params_cli_defaults()
    ws = [_window(rng, 118 + w, (100,), 64, extra_haps=30) for w in range(4)]
    pb = pack(ws)
    want = _oracle.batch(p, pb, nthreads=16)
    os.environ.update({"DD_DYNAMIC": "1", "DD_FORCE_GBT": gbt, "DD_TARGET_BLOCKS": "1000000"})
    got = run_host_api(lib, p, pb)
    assert any(l["n_haps"] * l["split"] > 2 * l["grid"] for l in capi.launch_log()), capi.launch_log()
    _assert_all_fields(got, want, pb, "persistent grid")
