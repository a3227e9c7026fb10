"""The N1 pair kernels (dd_pair_sum_kernel, dd_map_pair_kernel) on the directed cases of tests/_n1_cases.py: ragged
batches, caller-made ll, the read order bit for bit, the first-maximum rule at chosen lanes and passes, poisoned and
guarded outputs, a non-default stream.  Nothing here runs the HMM: the entry points take ll / pair_sum from the caller."""
import ctypes as C
import math

import numpy as np
import pytest

from dindel_tgi_amd import capi
from tests import _n1_cases as n1
from tests import _oracle
from tests.test_genotype_n1 import py_pair_posteriors

pytestmark = pytest.mark.gpu
GUARD = 64


def f64p(a):
    return a.ctypes.data_as(capi.c_f64p)


def nonempty(a):
    """A host array to point at: the library wants a non-null pointer even where it reads nothing."""
    return np.ascontiguousarray(a) if a.size else np.zeros(1, a.dtype)


def host_pair_sums(lib, pb, ll, n_slots):
    """dd_pair_sums into a sentinel-filled buffer with GUARD sentinels behind n_slots -> the n_slots it owns."""
    b = pb.ctypes_batch()
    out = np.full(n_slots + GUARD, n1.SENTINEL)
    assert lib.dd_pair_sums(C.byref(b), f64p(nonempty(ll)), f64p(out), 0) == 0, capi.last_error()
    assert (n1.bits(out[n_slots:]) == n1.bits(np.float64(n1.SENTINEL))).all()
    return out[:n_slots]


def oracle_sums(pb, ll, n_slots):
    b = pb.ctypes_batch()
    out = np.zeros(max(n_slots, 1))
    _oracle.load().ddo_pair_sums(C.byref(b), f64p(nonempty(ll)), f64p(out))
    return out[:n_slots]


def lower_triangle(shape):
    m = []
    for H, _ in shape:
        m += [h2 < h1 for h1 in range(H) for h2 in range(H)]
    return np.array(m, bool)


class DeviceArgs:
    """The three offset arrays of a dd_device_batch the N1 kernels read, win_hh_off and ll as torch tensors."""

    def __init__(self, pb, hh, ll):
        import torch
        self.torch = torch
        up = lambda a, dt: torch.from_numpy(np.array(a, dt)).cuda()           # a copy: the shared cases are read-only
        self.keep = [up(pb.a["win_hap_off"], np.int32), up(pb.a["win_read_off"], np.int32), up(pb.win_pair_off, np.int64)]
        self.hh = up(hh, np.int64)
        self.ll = up(ll, np.float64) if ll is not None else None
        self.ns = int(hh[-1])
        self.db = capi.dd_device_batch()
        self.db.n_windows = pb.n_windows
        self.db.win_hap_off, self.db.win_read_off, self.db.win_pair_off = (t.data_ptr() for t in self.keep)

    def guarded(self, n, dtype, fill):
        return self.torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")

    def pair_sums(self, lib, out, stream):
        rc = lib.dd_pair_sums_device(C.byref(self.db), self.hh.data_ptr(), self.ns, self.ll.data_ptr(), out.data_ptr(), stream.cuda_stream)
        assert rc == 0, capi.last_error()

    def map_pairs(self, lib, sums, prior, filt, ncand, post, pairs, vals, stream):
        rc = lib.dd_map_pairs_device(C.byref(self.db), self.hh.data_ptr(), sums.data_ptr(), prior.data_ptr(), filt.data_ptr(), ncand.data_ptr(),
                                     post.data_ptr() if post is not None else None, pairs.data_ptr(), vals.data_ptr(), stream.cuda_stream)
        assert rc == 0, capi.last_error()


def assert_guard(t, n, fill):
    tail = t[n:].cpu().numpy()
    want = np.full(GUARD, fill, tail.dtype)
    assert tail.tobytes() == want.tobytes(), "written behind the %d elements the kernel owns" % n


# ---- a) dd_pair_sums over shape lists x ll contents -------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(n1.SHAPES))
def test_pair_sums_matrix(lib, shape):
    """Per (shape list, ll contents): no sentinel survives in the slots the kernel owns and none is touched behind them;
    lower-triangle slots are exactly 0.0; finite slots are within 2 B of the oracle (B: tests/_n1_cases.py, derived from
    the arithmetic, not from this kernel); NaN slots are NaN exactly where the oracle has them; and every window's slots
    are bit-equal to the same window run alone, which a slot -> window search that lands on a neighbour cannot satisfy
    even where the neighbour's values are close."""
    low = lower_triangle(n1.SHAPES[shape])
    for kind in n1.CONTENTS:
        c = n1.case(shape, kind)
        pb, ll, hh, B = c["pb"], c["ll"], c["hh"], c["B"]
        ns = int(hh[-1])
        dev = host_pair_sums(lib, pb, ll, ns)
        assert not (n1.bits(dev) == n1.bits(np.float64(n1.SENTINEL))).any(), kind
        assert (n1.bits(dev[low]) == 0).all(), kind                          # +0.0, not merely == 0
        want = oracle_sums(pb, ll, ns)
        fin = np.isfinite(want)
        assert np.array_equal(np.isnan(dev), np.isnan(want)), kind
        assert np.array_equal(dev[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), kind
        err = np.abs(dev[fin] - want[fin])
        ratio = np.divide(err, B[fin], out=np.zeros_like(err), where=B[fin] > 0)
        print("%s/%s: max |dev - oracle| / B = %.3g" % (shape, kind, ratio.max() if ratio.size else 0.0))
        assert (err <= 2.0 * B[fin]).all(), (kind, np.flatnonzero(err > 2.0 * B[fin])[:8], ratio.max())
        for w, (H, R) in enumerate(c["shape"]):
            if H == 0:
                continue
            p0 = int(pb.win_pair_off[w])
            alone = host_pair_sums(lib, pb.slice_windows(w, w + 1), ll[p0:p0 + H * R], H * H)
            assert np.array_equal(n1.bits(alone), n1.bits(dev[hh[w]:hh[w + 1]])), (kind, w, H, R)


# ---- b) the read order, bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["host", "device"])
def test_pair_sums_add_in_read_order_bitwise(lib, entry):
    """Rows of U(-150, -5) against rows of -1e300: exp(-1e300) == 0 and log(1.0) == 0 exactly, each term is exactly
    log(1/2) + l[r], and the slot must equal the sequential fp64 sum in read order BIT FOR BIT (R = 63 .. 200).  The one
    thing taken from the device is its value of log(0.5), read from a probe slot of the same launch (an R = 1 window with
    ll = (0.0, -1e300)) and required to be within 1 ulp of math.log(0.5); everything else is computed here.  With that
    constant the reversed, wave-tree and exactly rounded sums of the same terms all give other bits (asserted), so a
    kernel that adds in another order, or drops or repeats a read of the last 64-block, fails.  (Adding the idle lanes of
    the last block as well is no error and cannot be seen: they hold 0.0, and x + 0.0 has the bits of x.)"""
    shape, ll, slots = n1.exact_case()
    pb, hh = n1.make_batch(shape), n1.slot_offsets(shape)
    ns = int(hh[-1])
    if entry == "host":
        dev = host_pair_sums(lib, pb, ll, ns)
    else:
        import torch
        d = DeviceArgs(pb, hh, ll)
        out = d.guarded(ns, torch.float64, n1.SENTINEL)
        torch.cuda.synchronize()
        d.pair_sums(lib, out, torch.cuda.current_stream())
        torch.cuda.synchronize()
        assert_guard(out, ns, n1.SENTINEL)
        dev = out[:ns].cpu().numpy()
    log5 = float(dev[n1.PROBE_SLOT])
    print("device log(0.5) = %r bits 0x%016x; math.log(0.5) = %r bits 0x%016x" %
          (log5, n1.bits1(log5), n1.LOG_HALF, n1.bits1(n1.LOG_HALF)))
    assert abs(n1.bits1(log5) - n1.bits1(n1.LOG_HALF)) <= 1
    for R in n1.EXACT_R:
        assert n1.order_sensitive(R, n1.EXACT_SEEDS[R], log5)
    for slot, row in slots:
        want = n1.seq_sum([log5 + x for x in row.tolist()])
        assert n1.bits1(dev[slot]) == n1.bits1(want), (slot, len(row), dev[slot], want)


# ---- c) device-pointer entries on torch tensors, a non-default stream, guarded outputs --------------------------------------
def map_inputs(pb, ns, seed):
    rng = np.random.default_rng(seed)
    prior = np.log(rng.choice([1e-4, 1e-3, 1.0], ns))
    filtered = (rng.random(pb.n_haps) < 0.15).astype(np.uint8)
    ncand = rng.integers(0, 2, pb.n_haps).astype(np.int32)
    return prior, filtered, ncand


def host_map_pairs(lib, pb, ll, prior, filtered, ncand, ns, want_sums=True, want_post=True):
    W = pb.n_windows
    b = pb.ctypes_batch()
    sums = np.full(ns + GUARD, n1.SENTINEL); post = np.full(ns + GUARD, n1.SENTINEL)
    pairs = np.full(4 * W + GUARD, n1.SENTINEL_I32, np.int32); vals = np.full(3 * W + GUARD, n1.SENTINEL)
    rc = lib.dd_map_pairs(C.byref(b), f64p(nonempty(ll)), f64p(nonempty(prior)), nonempty(filtered).ctypes.data_as(C.POINTER(C.c_uint8)),
                          nonempty(ncand).ctypes.data_as(capi.c_i32p), f64p(sums) if want_sums else None, f64p(post) if want_post else None,
                          pairs.ctypes.data_as(capi.c_i32p), f64p(vals), 0)
    assert rc == 0, capi.last_error()
    for a, n in ((sums, ns if want_sums else 0), (post, ns if want_post else 0), (vals, 3 * W)):
        assert (n1.bits(a[n:]) == n1.bits(np.float64(n1.SENTINEL))).all()
    assert (pairs[4 * W:] == n1.SENTINEL_I32).all()
    return sums[:ns], post[:ns], pairs[:4 * W], vals[:3 * W]


@pytest.mark.parametrize("shape,kind", [("ragged_2", "random"), ("ragged_3", "hap_minus_1e300"), ("single", "both_minus_inf")])
def test_device_entries_on_a_stream_with_guards(lib, shape, kind):
    """dd_pair_sums_device + dd_map_pairs_device as tools/n1_bench.py calls them, on a stream that is not the default one:
    bit-equal to the host-pointer entries, nothing written behind n_slots / 4 W / 3 W, every owned element written (the
    buffers start as sentinels), and a second launch into the same buffers gives the same bits."""
    import torch
    c = n1.case(shape, kind)
    pb, ll, hh = c["pb"], c["ll"], c["hh"]
    ns, W = int(hh[-1]), pb.n_windows
    prior, filtered, ncand = map_inputs(pb, ns, 11)
    h_sums, h_post, h_pairs, h_vals = host_map_pairs(lib, pb, ll, prior, filtered, ncand, ns)
    assert np.array_equal(n1.bits(h_sums), n1.bits(host_pair_sums(lib, pb, ll, ns)))
    d = DeviceArgs(pb, hh, ll)
    t_prior, t_filt, t_nc = torch.from_numpy(prior).cuda(), torch.from_numpy(filtered).cuda(), torch.from_numpy(ncand).cuda()
    sums, post = d.guarded(ns, torch.float64, n1.SENTINEL), d.guarded(ns, torch.float64, n1.SENTINEL)
    pairs, vals = d.guarded(4 * W, torch.int32, n1.SENTINEL_I32), d.guarded(3 * W, torch.float64, n1.SENTINEL)
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0 and side.cuda_stream != torch.cuda.default_stream().cuda_stream
    torch.cuda.synchronize()
    first = None
    for launch in range(2):
        d.pair_sums(lib, sums, side)
        d.map_pairs(lib, sums, t_prior, t_filt, t_nc, post, pairs, vals, side)
        side.synchronize()
        for t, n, fill in ((sums, ns, n1.SENTINEL), (post, ns, n1.SENTINEL), (pairs, 4 * W, n1.SENTINEL_I32), (vals, 3 * W, n1.SENTINEL)):
            assert_guard(t, n, fill)
        got = [sums[:ns].cpu().numpy(), post[:ns].cpu().numpy(), pairs[:4 * W].cpu().numpy(), vals[:3 * W].cpu().numpy()]
        if first is None:
            first = got
            for g, h in zip(got, (h_sums, h_post, h_pairs, h_vals)):
                assert g.tobytes() == h.tobytes()
            assert not (n1.bits(got[0]) == n1.bits(np.float64(n1.SENTINEL))).any()
            assert not (n1.bits(got[1]) == n1.bits(np.float64(n1.SENTINEL))).any()
        else:
            for g, f in zip(got, first):
                assert g.tobytes() == f.tobytes()


# ---- d) dd_map_pairs_device on given pair sums: indices exact ---------------------------------------------------------------
@pytest.mark.parametrize("sel", n1.SELECTIONS)
def test_map_pairs_first_maximum_tables(lib, sel):
    """pair_sum handed to dd_map_pairs_device directly (small integers: every pair_sum + prior is exact, a tie is a tie), one
    ragged launch per selection class with H = 1 .. 23, windows without haplotypes and W no multiple of 4.  Against
    py_pair_posteriors on the same arrays: pairs, posterior (0.0 in lower-triangle and filtered slots, which hold the
    largest pair_sum of all), vals[0] and vals[1] exact; qual as in test_genotype_n1.py (1e-12: device log / exp)."""
    import torch
    ws = n1.map_windows(sel)
    W = len(ws)
    assert W % 4 != 0
    shape = [(w[0], 0) for w in ws]
    pb, hh = n1.make_batch(shape), n1.slot_offsets(shape)
    ns = int(hh[-1])
    cat = lambda i, dt: np.ascontiguousarray(np.concatenate([w[i] for w in ws]), dt)
    ps, pr, f, nc = cat(1, np.float64), cat(2, np.float64), cat(3, np.uint8), cat(4, np.int32)
    d = DeviceArgs(pb, hh, None)
    t_ps, t_pr, t_f, t_nc = (torch.from_numpy(a).cuda() for a in (ps, pr, f, nc))
    post = d.guarded(ns, torch.float64, n1.SENTINEL)
    pairs, vals = d.guarded(4 * W, torch.int32, n1.SENTINEL_I32), d.guarded(3 * W, torch.float64, n1.SENTINEL)
    torch.cuda.synchronize()
    d.map_pairs(lib, t_ps, t_pr, t_f, t_nc, post, pairs, vals, torch.cuda.current_stream())
    torch.cuda.synchronize()
    for t, n, fill in ((post, ns, n1.SENTINEL), (pairs, 4 * W, n1.SENTINEL_I32), (vals, 3 * W, n1.SENTINEL)):
        assert_guard(t, n, fill)
    post, pairs, vals = post[:ns].cpu().numpy(), pairs[:4 * W].cpu().numpy(), vals[:3 * W].cpu().numpy()
    hoff = pb.a["win_hap_off"]
    for w, (H, wps, wpr, wf, wnc) in enumerate(ws):
        sl = slice(int(hh[w]), int(hh[w + 1]))
        want_post, pi, pn, mi, mn, qual = py_pair_posteriors(H, wps, wpr, wf, wnc)
        ctx = (sel, w, H)
        assert pairs[4 * w:4 * w + 4].tolist() == pi + pn, ctx
        nan = np.isnan(want_post)
        assert np.array_equal(np.isnan(post[sl]), nan), ctx
        assert np.array_equal(n1.bits(post[sl][~nan]), n1.bits(want_post[~nan])), ctx
        assert vals[3 * w] == mi and vals[3 * w + 1] == mn, ctx
        if math.isfinite(qual):
            assert vals[3 * w + 2] == pytest.approx(qual, rel=1e-12, abs=1e-12), ctx
        else:
            assert vals[3 * w + 2] == qual or (math.isnan(qual) and math.isnan(vals[3 * w + 2])), ctx
        assert int(hoff[w + 1] - hoff[w]) == H


def test_map_pairs_host_entry_without_haplotypes_and_without_optional_outputs(lib):
    """dd_map_pairs (host pointers): a batch in which no window has a haplotype gives rc 0, every pair -1 and
    vals = (-inf, -inf, NaN); posterior_out / pair_sum_out may be NULL and the rest is unchanged by that."""
    c = n1.case("all_h0", "random")
    W = c["pb"].n_windows
    _, _, pairs, vals = host_map_pairs(lib, c["pb"], c["ll"], np.zeros(0), np.zeros(0, np.uint8), np.zeros(0, np.int32), 0)
    assert pairs.tolist() == [-1] * (4 * W)
    v = vals.reshape(W, 3)
    assert (v[:, :2] == -math.inf).all() and np.isnan(v[:, 2]).all()
    c = n1.case("ragged_1", "random")
    ns = int(c["hh"][-1])
    prior, filtered, ncand = map_inputs(c["pb"], ns, 12)
    full = host_map_pairs(lib, c["pb"], c["ll"], prior, filtered, ncand, ns)
    assert not (n1.bits(full[0]) == n1.bits(np.float64(n1.SENTINEL))).any() and not (n1.bits(full[1]) == n1.bits(np.float64(n1.SENTINEL))).any()
    assert (np.array(full[2]).reshape(-1, 4)[np.array([H for H, _ in c["shape"]]) == 0] == -1).all()
    for want_sums, want_post in ((False, True), (True, False), (False, False)):
        part = host_map_pairs(lib, c["pb"], c["ll"], prior, filtered, ncand, ns, want_sums, want_post)
        assert part[2].tobytes() == full[2].tobytes() and part[3].tobytes() == full[3].tobytes()
        if want_sums:
            assert part[0].tobytes() == full[0].tobytes()
        if want_post:
            assert part[1].tobytes() == full[1].tobytes()
