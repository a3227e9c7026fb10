"""CPU-side checks of the certified MAP haplotype pair (dd_diploid_pair_result, dd_diploid_pairs_host, dd_diploid_pairs_device): declarations,
layout, validation, and the CPU evaluation against the real host function (maxLikelihoodPair's sums and argmax, through
ddh_max_likelihood_pair) on the windows of tests/_diploid_pair_cases.py — every certified window's pair is the host's — and on the
constructed cases, each of which must get its state; then a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np

from dindel_tgi_amd import capi
from dindel_tgi_amd.batch import alloc_result
from tests import _cigar_cases as cc
from tests import _diploid_pair_cases as dc
from tests import _host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dindel_tgi_amd", "host")
M, I, D, S = 0, 1, 2, 4
CSRC = os.path.join(ROOT, "dindel_tgi_amd", "csrc")
INF = np.inf


def test_header_compiles_as_c99_and_layout_agrees_with_ctypes(lib, tmp_path):
    src = tmp_path / "use_diploid_pairs.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dindel_hmm.h"\n'
                   'int main(void) {\n'
                   '  dd_diploid_pair_result c; (void)c;\n'
                   '  printf("%d %d %d %d %d %d\\n", (int)sizeof(dd_diploid_pair_result), (int)offsetof(dd_diploid_pair_result, pair),\n'
                   '         (int)offsetof(dd_diploid_pair_result, state), (int)offsetof(dd_diploid_pair_result, best),\n'
                   '         (int)offsetof(dd_diploid_pair_result, gap), (int)offsetof(dd_diploid_pair_result, margin));\n'
                   '  printf("%d %d %d %d %d %d %d %d\\n", DD_DIPPAIR_CERTIFIED, DD_DIPPAIR_TIE, DD_DIPPAIR_NONFINITE, DD_DIPPAIR_NOT_COMPUTED, DD_DIPPAIR_NO_HAPS,\n'
                   '         DD_DIPPAIR_TOO_MANY_HAPS, DD_DIPPAIR_MAX_HAPS, DD_ABI_VERSION);\n'
                   '  return dd_diploid_pairs_device(NULL, NULL, NULL, NULL, NULL, NULL, NULL) == DD_ERR_INVALID &&\n'
                   '         dd_diploid_pairs_host(NULL, NULL, NULL, NULL, NULL, 1) == DD_ERR_INVALID ? 0 : 1;\n}\n')
    exe = tmp_path / "use_diploid_pairs"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", CSRC, "-ldindel_hmm", "-Wl,-rpath," + CSRC, "-o", str(exe)])
    import torch
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    lines = subprocess.check_output([str(exe)], env=env).decode().splitlines()
    T = capi.dd_diploid_pair_result
    assert [int(v) for v in lines[0].split()] == [C.sizeof(T), T.pair.offset, T.state.offset, T.best.offset, T.gap.offset, T.margin.offset]
    assert [int(v) for v in lines[1].split()] == [capi.DD_DIPPAIR_CERTIFIED, capi.DD_DIPPAIR_TIE, capi.DD_DIPPAIR_NONFINITE, capi.DD_DIPPAIR_NOT_COMPUTED,
                                                  capi.DD_DIPPAIR_NO_HAPS, capi.DD_DIPPAIR_TOO_MANY_HAPS, capi.DD_DIPPAIR_MAX_HAPS, 13]
    assert capi.DD_DIPPAIR_CERTIFIED == 0 and capi.DD_DIPPAIR_MAX_HAPS >= 64
    assert lib.dd_abi_version() == 13 == capi.ABI_VERSION                      # new symbols only: the version is the parent's


def test_symbols_exist_and_the_helper_allocates_per_window(lib):
    for name in ("dd_diploid_pairs_device", "dd_diploid_pairs_host"):
        assert hasattr(lib, name) and name in capi.EXPORTS
    arrs, res = capi.diploid_pair_arrays(5)
    assert {k: (v.shape, v.dtype.name) for k, v in arrs.items()} == dict(pair=((5, 2), "int32"), state=((5,), "int32"), best=((5,), "float64"),
                                                                          gap=((5,), "float64"), margin=((5,), "float64"))
    assert res.pair == arrs["pair"].ctypes.data and res.margin == arrs["margin"].ctypes.data
    arrs0, res0 = capi.diploid_pair_arrays(0)                                   # an empty batch still has addresses to hand over
    assert len(arrs0["state"]) == 0 and res0.pair and res0.gap


def test_device_entry_validates_its_arguments(lib):
    db = capi.dd_device_batch()
    db.n_windows = 1
    db.win_hap_off = db.win_read_off = db.win_pair_off = 8                      # never dereferenced: every call below is refused first
    out = capi.dd_diploid_pair_result(8, 8, 8, 8, 8)
    ok = dict(b=C.byref(db), hh=8, ll=8, status=None, prior=8, out=C.byref(out))

    def call(**kw):
        a = dict(ok, **kw)
        return lib.dd_diploid_pairs_device(a["b"], a["hh"], a["ll"], a["status"], a["prior"], a["out"], None)
    for k in ("b", "hh", "ll", "prior", "out"):
        assert call(**{k: None}) == capi.DD_ERR_INVALID and "dd_diploid_pairs_device" in capi.last_error(), k
    for k in range(5):
        bad = [8] * 5
        bad[k] = 0
        assert call(out=C.byref(capi.dd_diploid_pair_result(*bad))) == capi.DD_ERR_INVALID
    for k in ("win_hap_off", "win_read_off", "win_pair_off"):
        db2 = capi.dd_device_batch()
        db2.n_windows = 1
        db2.win_hap_off = db2.win_read_off = db2.win_pair_off = 8
        setattr(db2, k, None)
        assert call(b=C.byref(db2)) == capi.DD_ERR_INVALID
    db.n_windows = -1
    assert call() == capi.DD_ERR_INVALID
    db.n_windows = 0                                                            # nothing to do: no launch, no device asked for
    assert call(hh=None, ll=None, prior=None) == 0


def test_host_evaluation_validates_its_arguments(lib):
    ho, ro = np.array([0, 2], np.int32), np.array([0, 3], np.int32)
    ll, prior = np.zeros(6), np.zeros(4)
    arrs, res = capi.diploid_pair_arrays(1)
    b = capi.dd_batch()
    b.n_windows, b.win_hap_off, b.win_read_off = 1, ho.ctypes.data_as(capi.c_i32p), ro.ctypes.data_as(capi.c_i32p)
    f = lib.dd_diploid_pairs_host
    llp, prp = ll.ctypes.data_as(capi.c_f64p), prior.ctypes.data_as(capi.c_f64p)
    assert f(C.byref(b), llp, None, prp, C.byref(res), 1) == 0 and arrs["state"][0] == capi.DD_DIPPAIR_TIE    # all zero: every pair the same
    assert f(None, llp, None, prp, C.byref(res), 1) == capi.DD_ERR_INVALID
    assert f(C.byref(b), llp, None, prp, None, 1) == capi.DD_ERR_INVALID
    assert f(C.byref(b), None, None, prp, C.byref(res), 1) == capi.DD_ERR_INVALID and "ll" in capi.last_error()
    assert f(C.byref(b), llp, None, None, C.byref(res), 1) == capi.DD_ERR_INVALID and "prior" in capi.last_error()
    for k in range(5):
        bad = [getattr(res, n) for n in capi.DIPLOID_PAIR_FIELDS]
        bad[k] = None
        assert f(C.byref(b), llp, None, prp, C.byref(capi.dd_diploid_pair_result(*bad)), 1) == capi.DD_ERR_INVALID
    down = np.array([3, 0], np.int32)
    b.win_read_off = down.ctypes.data_as(capi.c_i32p)
    assert f(C.byref(b), llp, None, prp, C.byref(res), 1) == capi.DD_ERR_INVALID and "decrease" in capi.last_error()
    b.n_windows = 0
    assert f(C.byref(b), None, None, None, C.byref(res), 4) == 0


def test_every_certified_window_has_the_hosts_pair_and_every_synthetic_window_is_certified():
    """The contract.  The synthetic windows' ll and priors are continuous, so a gap within the margin (~1e-9 at most) has negligible
    probability: all of them must be certified.  |V_twin - V_host| / eps over the certified windows' best pairs is printed and must be at
    most 1 (eps from the definition, with A summed in numpy; DESIGN 23 quotes the figure)."""
    c, tw, host = dc.build(), dc.twin(), dc.host()
    fuzz = np.flatnonzero(c["expect"] == dc.FUZZ)
    assert len(fuzz) >= 2000 and set(c["nh"][fuzz]) == set(range(1, 13)) | {65} and set(c["nr"][fuzz]) == set(dc.READ_COUNTS)
    assert (tw["state"][fuzz] == capi.DD_DIPPAIR_CERTIFIED).all(), np.bincount(tw["state"][fuzz])
    worst, n = 0.0, 0
    for w, (pair, V) in host.items():
        if tw["state"][w] != capi.DD_DIPPAIR_CERTIFIED:
            continue
        n += 1
        assert tuple(tw["pair"][w]) == pair, (w, tw["pair"][w], pair)
        ll, prior, _ = dc.window(c, w)
        h1, h2 = pair
        A = float(np.abs(np.logaddexp(ll[h1], ll[h2]) + np.log(0.5)).sum())
        R = ll.shape[1]
        eps = 2.0 ** -50 * ((R + 4) * A + 8 * R + abs(prior[h1, h2]))
        assert eps <= tw["margin"][w] * (1 + 1e-12)
        worst = max(worst, abs(tw["best"][w] - V[h1, h2]) / eps)
        assert (tw["margin"][w] < tw["gap"][w]) and tw["gap"][w] > 0
    print("certified windows: %d; max |V_twin - V_host| / eps = %.3g; smallest gap %.3g, largest margin %.3g"
          % (n, worst, tw["gap"][fuzz].min(), tw["margin"][fuzz].max()))
    assert n >= len(fuzz) and worst <= 1.0
    assert worst <= 0.5, "the bound is too thin: fix the bound"


def test_gap_is_the_distance_to_the_best_other_pair():
    """best and gap against the host's own values on a few windows: the runner-up is the largest V among the other pairs."""
    c, tw, host = dc.build(), dc.twin(), dc.host()
    for w in list(np.flatnonzero(c["expect"] == dc.FUZZ)[:200]) + [c["names"]["most_haplotypes"]]:
        pair, V = host[w]
        H = V.shape[0]
        vals = V[np.triu_indices(H)]
        if len(vals) == 1:
            assert tw["gap"][w] == INF
            continue
        top = np.sort(vals)[::-1]
        assert abs(tw["gap"][w] - (top[0] - top[1])) <= 2 * tw["margin"][w]
        assert abs(tw["best"][w] - top[0]) <= tw["margin"][w]


def test_constructed_cases_get_their_state_and_no_pair():
    c, tw = dc.build(), dc.twin()
    names = c["names"]
    for name, w in names.items():
        st, want = int(tw["state"][w]), int(c["expect"][w])
        assert st == want, (name, st, want)
        if st != capi.DD_DIPPAIR_CERTIFIED:
            assert tuple(tw["pair"][w]) == (-1, -1), name
        if st not in (capi.DD_DIPPAIR_CERTIFIED, capi.DD_DIPPAIR_TIE):
            assert tw["best"][w] == 0 and tw["gap"][w] == 0 and tw["margin"][w] == 0, name
    w = names["identical_columns"]
    assert tw["gap"][w] == 0.0 and tw["margin"][w] > 0
    w = names["ulp_apart"]
    _, V = dc.host()[w]
    d = (V[0, 1] - V[0, 0]) / np.spacing(abs(V[0, 0]))
    assert 1 <= d <= 4 and 0 <= tw["gap"][w] <= tw["margin"][w]                # the host sees 1 ... 4 ulp; the device does not decide
    w = names["one_haplotype"]
    assert tuple(tw["pair"][w]) == (0, 0) and tw["gap"][w] == INF
    w = names["no_reads"]
    assert tuple(tw["pair"][w]) == (0, 1) and tw["best"][w] == -2.5 and tw["gap"][w] == 0.25      # V is the prior
    w = names["most_haplotypes"]
    assert tuple(tw["pair"][w]) == dc.host()[w][0]
    for name in ("empty_first", "empty_between", "empty_last", "reads_without_haplotypes"):
        assert tw["state"][names[name]] == capi.DD_DIPPAIR_NO_HAPS
    seen = set(tw["state"].tolist())
    assert seen == set(range(6))


def test_threads_and_single_window_batches_change_nothing():
    c, tw = dc.build(), dc.twin()
    one = capi.diploid_pairs_host(c["ho"], c["ro"], c["ll"], c["prior"], c["status"], nthreads=1)
    for k in tw:
        assert np.array_equal(one[k], tw[k], equal_nan=True), k
    for w in list(c["names"].values()) + [3, 8, 100]:
        ll, prior, st = dc.window(c, w)
        got = capi.diploid_pairs_host([0, ll.shape[0]], [0, ll.shape[1]], ll.reshape(-1), prior.reshape(-1), st.reshape(-1))
        for k in tw:
            assert np.array_equal(got[k][0], tw[k][w]), (w, k)
    no_status = capi.diploid_pairs_host(c["ho"], c["ro"], c["ll"], c["prior"], None, nthreads=4)   # NULL status: every pair was computed
    w = c["names"]["status"]
    assert no_status["state"][w] == capi.DD_DIPPAIR_CERTIFIED and no_status["state"][c["names"]["status_before_nan"]] == capi.DD_DIPPAIR_NONFINITE


# ---------------------------------------------------------------- the host-pointer entry
def _host_call(lib, pb, ops_cap=8, prior="zeros", n_indels="zeros", hap_ref_pos="identity", options=0, with_hpos=True, pair_out="all", realign_out="all"):
    p = capi.params_cli_defaults()
    arrs, res = alloc_result(pb)
    if not with_hpos:
        res.hpos = None
    got, rl = capi.realign_arrays(pb.n_reads, max(ops_cap, 1))
    pairs, dp = capi.diploid_pair_arrays(pb.n_windows)
    if realign_out is None:
        rl = None
    elif realign_out != "all":
        setattr(rl, realign_out, None)
    if pair_out is None:
        dp = None
    elif pair_out != "all":
        setattr(dp, pair_out, None)
    nh = np.diff(pb.a["win_hap_off"]).astype(np.int64)
    pr = np.zeros(int((nh * nh).sum()) + 1) if isinstance(prior, str) else prior
    ni = np.zeros(pb.n_haps + 1, np.int32) if isinstance(n_indels, str) else n_indels
    hrp = np.arange(int(pb.a["hap_seq_off"][-1]), dtype=np.int32) if isinstance(hap_ref_pos, str) else hap_ref_pos
    b = pb.ctypes_batch()
    rc = lib.dd_compute_likelihoods_realign_diploid(C.byref(p), C.byref(b), C.byref(res), None if pr is None else pr.ctypes.data_as(capi.c_f64p),
                                                    None if ni is None else ni.ctypes.data_as(capi.c_i32p),
                                                    None if hrp is None else hrp.ctypes.data_as(capi.c_i32p), None, None if dp is None else C.byref(dp),
                                                    None if rl is None else C.byref(rl), ops_cap, 0, options)
    return rc, got, pairs


def test_host_entry_validates_and_has_no_cpu_fallback(lib):
    import torch
    assert hasattr(lib, "dd_compute_likelihoods_realign_diploid") and "dd_compute_likelihoods_realign_diploid" in capi.EXPORTS
    pb = cc.csr_batch([([30, 30], [20, 20])])
    rc, _, _ = _host_call(lib, pb, ops_cap=0)
    assert rc == capi.DD_ERR_INVALID and "ops_cap" in capi.last_error()
    rc, _, _ = _host_call(lib, pb, hap_ref_pos=None)
    assert rc == capi.DD_ERR_INVALID and "hap_ref_pos" in capi.last_error()
    rc, _, _ = _host_call(lib, pb, prior=None)
    assert rc == capi.DD_ERR_INVALID and "prior" in capi.last_error()
    rc, _, _ = _host_call(lib, pb, n_indels=None)
    assert rc == capi.DD_ERR_INVALID and "hap_n_indels" in capi.last_error()
    for out in (None, "hap", "status", "n_ops", "ops", "ref_off"):
        rc, _, _ = _host_call(lib, pb, realign_out=out)
        assert rc == capi.DD_ERR_INVALID and "dd_realign_result" in capi.last_error()
    for out in (None,) + capi.DIPLOID_PAIR_FIELDS:
        rc, _, _ = _host_call(lib, pb, pair_out=out)
        assert rc == capi.DD_ERR_INVALID and "dd_diploid_pair_result" in capi.last_error()
    rc, _, _ = _host_call(lib, pb, options=capi.DD_OPT_LONG_WINDOWS_FASTER)   # the main model's entry: only its own option bit
    assert rc == capi.DD_ERR_INVALID
    if not torch.cuda.is_available():
        for kw in (dict(), dict(with_hpos=False), dict(options=capi.DD_OPT_LONG_WINDOWS)):
            rc, _, _ = _host_call(lib, pb, **kw)
            assert rc == capi.DD_ERR_NO_DEVICE and "no CPU fallback" in capi.last_error()


def test_host_entry_on_a_batch_without_pairs_needs_no_device(lib):
    """No likelihood to take: the reads are marked, and the windows' states and pairs come from the priors alone (the CPU evaluation)."""
    pb = cc.csr_batch([([], [20, 20]), ([30, 30], []), ([], [])])
    prior = np.array([-3.0, -1.0, 0.0, -2.0, 0.0])
    rc, got, pairs = _host_call(lib, pb, prior=prior)
    assert rc == 0, capi.last_error()
    assert (got["status"] == capi.DD_REALIGN_NO_HAPS).all() and (got["hap"] == -1).all()
    assert list(pairs["state"]) == [capi.DD_DIPPAIR_NO_HAPS, capi.DD_DIPPAIR_CERTIFIED, capi.DD_DIPPAIR_NO_HAPS]
    assert pairs["pair"].tolist() == [[-1, -1], [0, 1], [-1, -1]] and pairs["best"][1] == -1.0 and pairs["gap"][1] == 1.0


# ---------------------------------------------------------------- the driver's switch
def test_driver_help_lists_the_switch_and_its_refusals():
    exe = os.path.join(HOST, "dindel_gpu")
    text = subprocess.check_output([exe, "--help"]).decode()
    assert "--deviceRealignDiploid" in text and "--checkDevicePair" in text and "--deviceRealign]" in text
    files = ["--outputRealignedBAM", "--bamFile", "x.bam", "--varFile", "w.txt", "--hapFile", "h.txt", "--outputFile", "o"]

    def refused(args, *words):
        r = subprocess.run([exe] + args + files, capture_output=True, text=True)
        lines = r.stderr.splitlines()
        assert r.returncode != 0 and r.stdout == "" and len(lines) == 1, (args, r.stderr)
        for w in words:
            assert w in lines[0], (args, lines[0])
    refused(["--deviceRealignDiploid", "--doDiploid", "--faster"], "--deviceRealignDiploid", "--faster")
    refused(["--deviceRealignDiploid"], "--deviceRealignDiploid", "--doDiploid")                       # the diploid step must be asked for by name
    refused(["--deviceRealignDiploid", "--doPooled"], "--deviceRealignDiploid", "--doDiploid")
    refused(["--deviceRealignDiploid", "--doDiploid", "--doPooled", "--deviceRealign"], "--deviceRealign")
    refused(["--deviceRealign", "--doDiploid", "--doPooled"], "--deviceRealign", "--doDiploid")        # the existing refusal stands
    r = subprocess.run([exe, "--deviceRealignDiploid", "--faster"], capture_output=True, text=True)    # said before anything else is asked for
    assert r.returncode != 0 and len(r.stderr.splitlines()) == 1 and "--deviceRealignDiploid" in r.stderr


# ---------------------------------------------------------------- the consumer of the views, on hand-made ones
def _consume(rows, state, pair, ll, H=3, read_len=12, hap_len=40, ops_cap=2, hpos=None, ref_seq_pos=1000, max_ops=4):
    """rows: per read (hap, status, [BAM words], ref_off, n_ops or None = len(words)) -> dict(rc, n, pos, ops, fallbacks, uncertified, used, msg)."""
    f = _host.load().ddh_diploid_device_realigned_cigars
    f.argtypes = [C.c_int] * 6 + [C.c_void_p] * 8 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.POINTER(C.c_long), C.POINTER(C.c_long), C.c_void_p, C.c_char_p, C.c_int]
    f.restype = C.c_int
    R = len(rows)
    hap = np.array([r[0] for r in rows], np.int32)
    status = np.array([r[1] for r in rows], np.int32)
    ops = np.zeros((R, ops_cap), np.uint32)
    for i, r in enumerate(rows):
        ops[i, :min(len(r[2]), ops_cap)] = r[2][:ops_cap]
    ref_off = np.array([r[3] for r in rows], np.int32)
    n_ops = np.array([len(r[2]) if len(r) < 5 else r[4] for r in rows], np.int32)
    out_n, out_pos, out_ops = np.full(R, -7, np.int32), np.full(R, -7, np.int32), np.full((R, max_ops), 0xFFFFFFFF, np.uint32)
    fb, un, err, used = C.c_long(-1), C.c_long(-1), C.create_string_buffer(200), np.full(2, -9, np.int32)
    hp = None if hpos is None else np.ascontiguousarray(hpos, np.int16)
    assert hp is None or hp.shape == (H, R, read_len)
    llv = np.ascontiguousarray(ll, np.float64)
    assert llv.shape == (H, R)
    pr = np.array(pair, np.int32)
    rc = f(H, R, read_len, hap_len, ops_cap, state, pr.ctypes.data, llv.ctypes.data, hap.ctypes.data, status.ctypes.data, n_ops.ctypes.data, ops.ctypes.data,
           ref_off.ctypes.data, None if hp is None else hp.ctypes.data, ref_seq_pos, out_n.ctypes.data, out_pos.ctypes.data, out_ops.ctypes.data, max_ops,
           C.byref(fb), C.byref(un), used.ctypes.data, err, 200)
    return dict(rc=rc, n=out_n, pos=out_pos, ops=out_ops, fallbacks=fb.value, uncertified=un.value, used=tuple(used), msg=err.value.decode())


def w(op, ln):
    return (ln << 4) | op


def _gapped_hpos(H, R, L):
    hpos = np.zeros((H, R, L), np.int16)
    for h in range(H):
        for r in range(R):
            v = np.arange(L) + h + r
            v[L // 2:] += 2                                                         # two haplotype bases deleted: 6M2D6M on the identity map
            hpos[h, r] = v
    return hpos


def test_consumer_takes_a_certified_windows_rows_as_they_are():
    """Nothing of the pair choice is computed on the host: the likelihoods say (2, 2), the device said (0, 1), and (0, 1) it is."""
    ll = np.array([[-9.0] * 3, [-8.0] * 3, [-1.0] * 3])
    rows = [(1, capi.DD_CIGAR_OK, [w(M, 12)], 13), (0, capi.DD_CIGAR_OK, [w(S, 2), w(M, 10)], 21), (1, capi.DD_CIGAR_OK, [w(S, 12)], -1)]
    got = _consume(rows, capi.DD_DIPPAIR_CERTIFIED, (0, 1), ll)
    assert got["rc"] == 0 and got["fallbacks"] == 0 and got["uncertified"] == 0 and got["used"] == (0, 1), got["msg"]
    assert list(got["n"]) == [1, 2, 1] and list(got["pos"]) == [1013, 1021, -1]
    assert list(got["ops"][0]) == [w(M, 12), 0, 0, 0] and list(got["ops"][1]) == [w(S, 2), w(M, 10), 0, 0]
    bad = _consume(rows[:2] + [(2, capi.DD_CIGAR_OK, [w(M, 12)], 0)], capi.DD_DIPPAIR_CERTIFIED, (0, 1), ll)      # a haplotype outside the pair
    assert bad["rc"] == -1 and "no haplotype of its pair" in bad["msg"]
    bad = _consume(rows[:2] + [(-1, capi.DD_REALIGN_BAD_PAIR, [], -1)], capi.DD_DIPPAIR_CERTIFIED, (0, 1), ll)
    assert bad["rc"] == -1 and "no haplotype of its pair" in bad["msg"]
    thrown = _consume(rows[:1] + [(0, capi.DD_CIGAR_ERROR2, [], -1)], capi.DD_DIPPAIR_CERTIFIED, (0, 1), ll[:, :2])
    assert thrown["rc"] == -1 and thrown["msg"] == capi.CIGAR_MESSAGES[capi.DD_CIGAR_ERROR2]


def test_consumer_redoes_a_certified_windows_reads_over_the_cap_on_the_host():
    H, R, L = 3, 3, 12
    ll = np.zeros((H, R))
    hpos = _gapped_hpos(H, R, L)
    rows = [(2, capi.DD_CIGAR_OVERFLOW, [w(M, 6), w(D, 2)], 20, 3), (0, capi.DD_CIGAR_OK, [w(M, 12)], 1), (2, capi.DD_CIGAR_NOT_COMPUTED, [], -1, 0)]
    got = _consume(rows, capi.DD_DIPPAIR_CERTIFIED, (0, 2), ll, hpos=hpos)
    assert got["rc"] == 0 and got["fallbacks"] == 2 and got["uncertified"] == 0 and got["used"] == (0, 2), got["msg"]
    assert list(got["n"]) == [3, 1, 3] and list(got["ops"][0]) == [w(M, 6), w(D, 2), w(M, 6), 0] and list(got["ops"][2]) == list(got["ops"][0])
    assert list(got["pos"]) == [1000 + 20 + 2 + 0, 1001, 1000 + 20 + 2 + 2]         # haplotype h lies at 10 h; the read starts at base h + r
    none = _consume(rows, capi.DD_DIPPAIR_CERTIFIED, (0, 2), ll, hpos=None)
    assert none["rc"] == -1 and "no alignments are at hand" in none["msg"]


def test_consumer_sends_an_uncertified_window_through_the_host():
    """Any state but certified: maxLikelihoodPair on the view's likelihoods, then the host's CIGARs for that pair from the alignments; the
    device's rows (DD_REALIGN_BAD_PAIR) are not looked at.  The window is counted, its reads are not per-read fallbacks."""
    H, R, L = 3, 4, 12
    hpos = _gapped_hpos(H, R, L)
    ll = np.array([[-30.0, -31.0, -29.0, -30.0], [-2.0, -9.0, -2.5, -9.0], [-9.0, -1.0, -9.0, -1.5]])    # reads 0, 2 from haplotype 1; 1, 3 from 2
    rows = [(-1, capi.DD_REALIGN_BAD_PAIR, [], -1)] * R
    for state in (capi.DD_DIPPAIR_TIE, capi.DD_DIPPAIR_NONFINITE, capi.DD_DIPPAIR_NOT_COMPUTED, capi.DD_DIPPAIR_TOO_MANY_HAPS):
        got = _consume(rows, state, (-1, -1), ll, hpos=hpos)
        assert got["rc"] == 0 and got["uncertified"] == 1 and got["fallbacks"] == 0 and got["used"] == (1, 2), got["msg"]
        assert list(got["n"]) == [3] * R
        assert list(got["pos"]) == [1000 + 10 * h + h + r for r, h in enumerate([1, 2, 1, 2])]           # each read on the likelier of the two
    none = _consume(rows, capi.DD_DIPPAIR_TIE, (-1, -1), ll, hpos=None)
    assert none["rc"] == -1 and "no alignments are at hand" in none["msg"]


def test_check_program_under_address_and_undefined_sanitizers(tmp_path):
    """tests/diploid_pair_check.cpp with the CPU evaluation, the adapter, the consumer and the units they stand on, g++ alone (the rest of the C
    ABI is stubbed in the program), under AddressSanitizer and UBSan; run directly."""
    exe = str(tmp_path / "diploid_pair_check")
    units = ["compute_likelihoods", "device_pair", "realigned_bam", "cigar", "genotype", "diploid_glf", "bam_reader", "fast_inflate"]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-ffp-contract=off", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DDD_DIPLOID_PAIR_STANDALONE", "-o", exe, os.path.join(ROOT, "tests", "diploid_pair_check.cpp"),
                           os.path.join(CSRC, "diploid_pair_host.cpp")] + [os.path.join(HOST, u + ".cpp") for u in units] + ["-lz"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.endswith("diploid_pair_check: ok\n") and r.stderr == "", (r.stdout[-2000:], r.stderr[-4000:])
