"""dd_pooled_em (pooled_em_kernel.hip) against dd_pooled_em_host: every output bit for bit, iteration counts included.  No tolerance:
both sides evaluate csrc/pooled_math.h in one order.  dd_pooled_em_host itself is compared with exact arithmetic in
tests/test_pooled_em_cpu.py."""
import numpy as np
import pytest

from dindel_tgi_amd import capi, pooled, synth

pytestmark = pytest.mark.gpu
READS = [0, 1, 2, 63, 64, 65, 128, 130, 1000]
HAPS = [1, 2, 8, 9, 33, 200]
MASKS = ["all", "one", "alternating"]
CONTENTS = ["random", "read_row_minus_1e4", "all_equal", "haplotype_minus_1e300"]


def mask(kind, nh, k=0):
    if kind == "all":
        return [1] * nh
    if kind == "one":
        return [1 if h == (k % nh) else 0 for h in range(nh)]
    return [1 if h % 2 == 0 else 0 for h in range(nh)]


def window_ll(rng, content, nh, nr):
    """One window's ll, haplotype-major [nh, nr]."""
    if content == "all_equal":
        return np.full((nh, nr), -20.0)
    ll = rng.uniform(-150.0, -5.0, size=(nh, nr))
    if content == "read_row_minus_1e4" and nr:
        ll[:, nr // 2] = -1e4
    if content == "haplotype_minus_1e300":
        ll[nh - 1, :] = -1e300
    return ll


def grid_batch(content, seed):
    rng = np.random.default_rng(seed)
    shapes = [(nh, nr) for nh in HAPS for nr in READS]
    who = np.concatenate([[0], np.cumsum([s[0] for s in shapes])]).astype(np.int32)
    wro = np.concatenate([[0], np.cumsum([s[1] for s in shapes])]).astype(np.int32)
    ll = np.concatenate([window_ll(rng, content, nh, nr).reshape(-1) for nh, nr in shapes] + [np.zeros(0)])
    sw, compat = [], []
    for w, (nh, nr) in enumerate(shapes):
        for k, m in enumerate(MASKS):
            sw.append(w)
            compat.append(mask(m, nh, w + k))
    return who, wro, ll, pooled.pack_slots(who, sw, compat)


def assert_same_bits(got, want):
    for k in ("iters", "loglik", "ediff", "freqs"):
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape, k
        same = g.view(np.uint8).reshape(len(g), -1) == w.view(np.uint8).reshape(len(w), -1) if len(g) else np.ones((0, 1), bool)
        bad = np.flatnonzero(~same.all(axis=1))
        assert len(bad) == 0, (k, len(bad), bad[:5], g[bad[:5]], w[bad[:5]])
        assert np.array_equal(g, w, equal_nan=True), k


@pytest.mark.parametrize("a0", [0.001, 1.0])
@pytest.mark.parametrize("content", CONTENTS)
def test_grid_bit_equal(lib, content, a0):
    """Every R x H of the grid as one ragged batch, three masks per window."""
    who, wro, ll, slots = grid_batch(content, seed=CONTENTS.index(content) * 2 + int(a0 == 1.0))
    want = pooled.em_host(who, wro, ll, slots, a0=a0, tol=1e-4, nthreads=16)
    got = pooled.em(who, wro, ll, slots, a0=a0, tol=1e-4)
    assert (want["iters"] >= 2).all() and (want["iters"] <= 27).all()
    assert_same_bits(got, want)


def close_batch(seed, shapes):
    """Windows whose haplotypes explain the reads about equally well: the EM takes many iterations."""
    rng = np.random.default_rng(seed)
    who = np.concatenate([[0], np.cumsum([s[0] for s in shapes])]).astype(np.int32)
    wro = np.concatenate([[0], np.cumsum([s[1] for s in shapes])]).astype(np.int32)
    ll = np.concatenate([(rng.uniform(-150, -5, size=(1, nr)) + rng.uniform(-1.5, 1.5, size=(nh, nr))).reshape(-1) for nh, nr in shapes])
    return who, wro, ll


def test_iteration_cap(lib):
    """tol = 0: |eOld - eNew| < 0 never holds, the loop ends at the cap of 27 iterations on both sides."""
    shapes = [(3, 40), (8, 130), (2, 64), (9, 0), (33, 65)]
    who, wro, ll = close_batch(5, shapes)
    slots = pooled.pack_slots(who, list(range(len(shapes))), [mask("all", nh) for nh, _ in shapes])
    want = pooled.em_host(who, wro, ll, slots, tol=0.0)
    got = pooled.em(who, wro, ll, slots, tol=0.0)
    assert (want["iters"] == 27).all()
    assert_same_bits(got, want)


def test_quick_convergence_and_many_iterations(lib):
    """One slot that converges within three iterations (one compatible haplotype) beside slots that need many."""
    shapes = [(4, 70), (4, 70), (3, 200), (8, 1000)]
    who, wro, ll = close_batch(6, shapes)
    slots = pooled.pack_slots(who, [0, 1, 2, 3], [mask("one", 4, 2), mask("all", 4), mask("all", 3), mask("all", 8)])
    want = pooled.em_host(who, wro, ll, slots, nthreads=4)
    got = pooled.em(who, wro, ll, slots)
    assert want["iters"][0] <= 3 and want["iters"][1:].max() > 3, want["iters"]
    assert_same_bits(got, want)


def test_ragged_slot_table(lib):
    """Windows that differ in reads, haplotypes and number of sets, slots not in window order, one window without a slot."""
    shapes = [(2, 10), (5, 67), (1, 3), (9, 129), (4, 0), (3, 64)]
    who, wro, ll = close_batch(7, shapes)
    sw = [3, 0, 0, 5, 1, 1, 1, 4, 3, 3, 3, 3, 0]
    compat = [mask(MASKS[k % 3], shapes[w][0], k) for k, w in enumerate(sw)]
    slots = pooled.pack_slots(who, sw, compat)
    want = pooled.em_host(who, wro, ll, slots, a0=0.5, nthreads=3)
    got = pooled.em(who, wro, ll, slots, a0=0.5)
    assert_same_bits(got, want)
    # and each slot equals the same slot run alone
    for k, w in enumerate(sw):
        alone = pooled.em(who, wro, ll, pooled.pack_slots(who, [w], [compat[k]]), a0=0.5)
        o = int(slots["slot_off"][k])
        assert alone["loglik"][0] == got["loglik"][k] and alone["iters"][0] == got["iters"][k]
        assert np.array_equal(alone["freqs"], got["freqs"][o:o + shapes[w][0]])


@pytest.mark.parametrize("faster", [False, True])
def test_on_resident_ll(lib, faster):
    """The EM behind DeviceBatch.launch() / launch_faster(), on the ll in HBM: the same bits as dd_pooled_em on the ll copied back."""
    from dindel_tgi_amd.device import DeviceBatch
    pb = synth.generate(5, H=4, R=70, L=100, hap_len=120, seed=11)
    dev = DeviceBatch(pb, capi.params_cli_defaults(), "cuda:0")
    who, wro = pb.a["win_hap_off"], pb.a["win_read_off"]
    sw = [w for w in range(pb.n_windows) for _ in range(2)]
    compat = [mask(MASKS[k % 3], int(who[w + 1] - who[w]), k) for k, w in enumerate(sw)]
    slots = pooled.pack_slots(who, sw, compat)
    (dev.launch_faster if faster else dev.launch)()
    dev.pooled_em(slots)
    got = dev.pooled_em_results()
    ll = dev.results()["ll"]
    assert np.isfinite(ll).all() and (ll < 0).all()
    assert_same_bits(got, pooled.em(who, wro, ll, slots))
    assert_same_bits(got, pooled.em_host(who, wro, ll, slots))


def test_invalid_arguments(lib):
    who, wro = np.array([0, 2], np.int32), np.array([0, 3], np.int32)
    slots = pooled.pack_slots(who, [0], [[1, 1]])
    with pytest.raises(RuntimeError):
        pooled.em(who, wro, np.full(6, -10.0), slots, a0=-1.0)
    with pytest.raises(RuntimeError):
        pooled.em(who, wro, np.full(6, -10.0), dict(slots, slot_off=np.array([0, 3], np.int64)))
