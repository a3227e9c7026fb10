"""The long scenario batches of tests/_path_scenarios.py (long_batch_for) reach what tests/test_gpu_long_path_matrix.py and
tests/test_gpu_faster_path_matrix.py claim for them — shown on the oracle, dd_screen_windows_ex and host arithmetic alone, for every case
of those matrices.  No device.

Per case: every window is DD_WIN_LONG but the three that must not be; the reach properties of tests/test_path_scenarios_cpu.py; the K the
case is meant for; more pairs (16-pair items) than the persistent grid can have workgroups; and the fixed number of pairs a comparison
leaves out, so that a change to the builder cannot quietly grow what is skipped."""
import functools

import numpy as np
import pytest

from dindel_tgi_amd import capi
from tests import _oracle
from tests import _path_scenarios as ps

CASES = [pytest.param(hl, L, mld, K, id="hap%d-L%d-mld%d-K%d" % (hl, L, mld, K)) for hl, L, mld, K in ps.LONG_GRID]
FASTER_CASES = [pytest.param(hl, L, mld, id="hap%d-L%d-mld%d" % (hl, L, mld)) for hl, L, mld in ps.FASTER_LONG_GRID]
N_REJECTED, N_HAPSIZE, N_FASTER_NAN = 2, 6, 8          # pairs of the window with the empty read; reads on the 4-bp haplotype; see below
# The longest deletion a most likely path can hold under params_for: one deletion of n bases costs log(1e-5) - (n - 1) / 2 (the oracle's
# pass_two_inc: logProbError off a homopolymer, logpInsgIns per further base), -24.5 at n = 27, and the path that leaves the read's middle
# base off the haplotype costs no less than the Phred-100 cap of the mapping quality, log(1e-10) = -23.0 (the ladder reads have ll -9.8 there,
# -23.6 at the cap).  So at maxLengthDel 31 the jump lengths 27 .. 31 are candidates that every state evaluates and that lose: the ladder
# holds one indel each up to 26 and the reads above it are off the haplotype.  (maxLengthDel 5, 11 and 20: the whole ladder, as on the main grid.)
LADDER_MAX = 26


@functools.lru_cache(maxsize=None)
def point(hl, L, mld):
    """(PackedBatch, index, oracle arrays with mapUnmappedReads = 1) of the case's batch with both extra windows, computed once."""
    pb, index = ps.long_batch_for(hl, L, mld, wide=True, many=True)
    return pb, index, _oracle.batch(ps.params_for(mld), pb, nthreads=16)


def test_long_grid_sits_on_both_sides_of_every_k_bound():
    for K in (1, 2, 4, 8, 16):
        mine = [c for c in ps.LONG_GRID if c[3] == K]
        assert sorted(c[0] for c in mine) == [120 if K == 1 else 128 * K - 1, 256 * K - 2]
        assert min(c[2] for c in mine) <= 11 and max(c[2] for c in mine) >= 12 and sorted(c[1] for c in mine) == [36, 100]
    assert {c[2] for c in ps.LONG_GRID} == {5, 11, 20, 31}
    assert max(c[0] for c in ps.LONG_GRID) == capi.DD_LONG_MAX_HAP_LEN
    assert ps.long_grid_bound(4094, ps.LONG_WIDE_LEN) == (16, 31) and ps.long_grid_bound(2046, ps.LONG_WIDE_LEN) == (8, 63)
    assert ps.long_grid_bound(1022, ps.LONG_WIDE_LEN) == (4, 127) and ps.long_grid_bound(510, ps.LONG_WIDE_LEN) == (2, 255)
    assert ps.long_grid_bound(254, ps.LONG_WIDE_LEN) == (1, 510) and ps.long_grid_bound(4094, ps.LONG_FORCE_LEN) == (16, 125)


@pytest.mark.parametrize("hl,L,mld,K", CASES)
def test_builder_is_a_function_of_its_arguments_and_wide_only_appends(hl, L, mld, K):
    a, ia = ps.long_batch_for(hl, L, mld, wide=True, many=True)
    b, ib = point(hl, L, mld)[:2]
    assert all(np.array_equal(a.a[k], b.a[k]) for k in a.a) and all(np.array_equal(ia[k], ib[k]) for k in ia)
    assert np.array_equal(a.hap_var_flank, b.hap_var_flank) and all(np.array_equal(a.mate[k], b.mate[k]) for k in a.mate)
    n, i_n = ps.long_batch_for(hl, L, mld, wide=False, many=True)                    # the batch without the last window, array for array
    assert n.n_windows == a.n_windows - 1 and n.n_pairs == a.n_pairs - 1
    for k in n.a:
        if k in ("qual_table", "mapq_table"):
            assert np.array_equal(n.a[k], a.a[k]), k                                   # the wide read brings no new quality
        else:
            assert np.array_equal(n.a[k], a.a[k][:len(n.a[k])]), k
    assert np.array_equal(n.hap_var_flank, a.hap_var_flank[:len(n.hap_var_flank)])
    assert all(np.array_equal(i_n[k], ia[k]) for k in i_n) and set(ia) - set(i_n) == {"long.wide"}
    assert len(ia["long.wide"]) == 1 and int(ia["long.wide"][0]) == a.n_pairs - 1
    r = np.diff(a.a["read_seq_off"])
    assert r[-1] == ps.LONG_WIDE_LEN and (r == ps.LONG_WIDE_LEN).sum() == 1 and (len(ia["long.many"]) // 2 + 1) % 16


@pytest.mark.parametrize("hl,L,mld,K", CASES)
def test_every_window_is_long_but_the_three_that_must_not_be(lib, hl, L, mld, K):
    pb, index, want = point(hl, L, mld)
    p = ps.params_for(mld)
    H, R = np.diff(pb.a["win_hap_off"]), np.diff(pb.a["win_read_off"])
    rl = np.diff(pb.a["read_seq_off"])
    empty = np.array([(rl[pb.a["win_read_off"][w]:pb.a["win_read_off"][w + 1]] == 0).any() for w in range(pb.n_windows)])
    stay = (H == 0) | (R == 0) | empty
    assert stay.sum() == 3 and (H[stay] == 0).sum() == 1 and (R[stay] == 0).sum() == 1 and empty.sum() == 1
    cls, mx, n_bad = capi.screen_windows_ex(p, pb)
    assert (cls[~stay] == capi.DD_WIN_LONG).all() and n_bad == 1, cls
    assert cls[empty][0] == capi.DD_WIN_UNSUPPORTED and (cls[stay & ~empty] == capi.DD_WIN_MAIN).all()
    assert mx[2] == hl and mx[3] == ps.LONG_WIDE_LEN
    cls0, _mx, n_bad0 = capi.screen_windows_ex(p, pb, 0)                               # without the option: the three as before, no long window
    assert np.array_equal(cls0[stay], cls[stay]) and (cls0[~stay] == capi.DD_WIN_UNSUPPORTED).all() and n_bad0 == pb.n_windows - 2
    clsf, _mx, _n = capi.screen_windows_ex(p, pb, capi.DD_OPT_LONG_WINDOWS_FASTER)     # the --faster model's screen: the same classes
    assert np.array_equal(clsf, cls)
    # every forced window has exactly one read of 1,025 bp, its last; the wide window's one read is the only longer one
    for w in np.nonzero(~stay)[0][:-1]:
        mine = rl[pb.a["win_read_off"][w]:pb.a["win_read_off"][w + 1]]
        assert mine[-1] == ps.LONG_FORCE_LEN and (mine[:-1] <= capi.DD_MAX_READ_LEN).all(), w
    assert len(index["long.force"]) == int(H[~stay][:-1].sum())
    # the K the case is meant for; the hapSize window's 80-bp haplotype rides on it
    numS = int(np.diff(pb.a["hap_seq_off"]).max()) + 2
    assert numS == hl + 2 and numS <= 256 * K and (K == 1 or numS > 128 * K)
    assert ps.long_grid_bound(hl, ps.LONG_FORCE_LEN)[0] == K
    w = int(np.searchsorted(pb.win_pair_off, index["screened.hapsize"][0], side="right")) - 1
    h0 = int(pb.a["win_hap_off"][w])
    assert np.diff(pb.a["hap_seq_off"])[h0:h0 + 2].tolist() == [min(80, hl), 4] and cls[w] == capi.DD_WIN_LONG
    # more than twice the pairs the persistent grid can have workgroups, with and without the wide window
    pairs, _items = ps.long_pairs(pb, cls)
    assert pairs - 1 > 2 * ps.long_grid_bound(hl, ps.LONG_FORCE_LEN)[1] and ps.long_grid_bound(hl, ps.LONG_FORCE_LEN)[1] >= ps.long_grid_bound(hl, ps.LONG_WIDE_LEN)[1]


@pytest.mark.parametrize("hl,L,mld,K", CASES)
def test_the_reach_properties_of_the_main_scenarios_hold(hl, L, mld, K):
    pb, index, want = point(hl, L, mld)
    ll = want["ll"]
    assert (ll[index["redo"]] < -99).sum() >= 4 and (ll[index["redo.ordinary"]] > -99).sum() >= 4, (ll[index["redo"]], ll[index["redo.ordinary"]])
    nind = want["numIndels"][index["ends.ladder"]]
    assert len(nind) == mld + 1 and (nind[:min(mld, LADDER_MAX)] == 1).all(), nind    # one deletion each, lengths 1 .. maxLengthDel
    assert not nind[LADDER_MAX:mld].any() and want["offHap"][index["ends.ladder"][LADDER_MAX:mld]].all()
    assert want["offHap"][index["ends.ladder"][mld]] == 1 or nind[mld] != 1
    hp = want["hpos"][:pb.hpos_len]
    assert (hp == capi.DD_HPOS_LO).any() and (hp == capi.DD_HPOS_RO).any() and (hp <= capi.DD_HPOS_INS_KEY0).any()
    rl = np.diff(pb.a["read_seq_off"])
    assert 1 in rl and 2 in rl and 0xFFFFFFFF in pb.a["read_start"] and 3 in pb.a["read_start"] and (pb.a["read_flags"] & 1).any()
    for k in ("var_covered", "var_fcov"):
        assert set(np.unique(want[k][:pb.var_cov_len]).tolist()) == {0, 1}, k
    assert set(pb.hap_var_flank[2::3].tolist()) == {1, 2}
    assert pb.ctypes_batch().n_qual == 256 and len(np.unique(pb.a["qual_table"])) == 256
    assert set(np.unique(want["offHap"][index["quals"]]).tolist()) == {0, 1}
    hb, rb = set(pb.a["hap_seq"].tobytes().decode()), set(pb.a["read_seq"].tobytes().decode())
    assert {"N", "R", "a", "n"} <= hb and {"N", "R", "n", "Y"} <= rb
    haps = pb.a["hap_seq"].tobytes().decode()
    assert "AC" * 6 in haps and "CAG" * 4 in haps and "T" * 12 in haps and "A" * hl in haps and "NNN" in haps
    assert want["numMismatch"][index["bytes"]].any()
    # the forced reads are computed like any other (one is on the 4-bp haplotype: hapSize error)
    assert (want["status"][index["long.force"]] != capi.DD_PAIR_OK).sum() == 1 and want["status"][index["long.wide"]][0] == capi.DD_PAIR_OK
    assert ("chunk" not in index or index["chunk"].size == 0) and index["long.many"].size >= 74


@pytest.mark.parametrize("hl,L,mld,K", CASES)
def test_mate_prior_moves_the_pairs_with_a_usable_mate_only(hl, L, mld, K):
    pb, index, want = point(hl, L, mld)
    w = int(index["mates.window"][0])
    off = _oracle.batch(ps.params_for(mld, 0), pb, first_window=w, n_win=1)
    use, not_use = index["mates.usable"], index["mates.unusable"]
    assert len(use) + len(not_use) == 22 * 3 and len(use) >= 6 * 3
    assert (want["ll"][use] != off["ll"][use]).any()
    assert np.array_equal(want["ll"][not_use], off["ll"][not_use])
    mine = np.arange(int(pb.win_pair_off[w]), int(pb.win_pair_off[w + 1]))
    forced = np.intersect1d(mine, index["long.force"])                                 # the window's 1,025-bp read is unpaired: no prior term
    assert len(forced) == 3 and np.array_equal(want["ll"][forced], off["ll"][forced])


@pytest.mark.parametrize("hl,L,mld,K", CASES)
def test_what_a_comparison_leaves_out_is_fixed(hl, L, mld, K):
    """Main model: the two pairs of the rejected window (the library defines four of their values, tests/_path_scenarios.with_screened)
    and the hpos of the six hapSize-error pairs; everything else is compared bit for bit."""
    pb, index, want = point(hl, L, mld)
    st = want["status"][:pb.n_pairs]
    rej, hs = index["screened.rejected"], index["screened.hapsize"]
    assert len(rej) == N_REJECTED and len(hs) == N_HAPSIZE and (st[hs] == capi.DD_PAIR_HAPSIZE).all()
    rest = np.ones(pb.n_pairs, bool)
    rest[rej] = False
    rest[hs] = False
    assert (st[rest] == capi.DD_PAIR_OK).all() and rest.sum() == pb.n_pairs - 8
    got, exp = ps.with_screened(want, want, pb, index)                                 # the library's defined values replace the oracle's there only
    for k in want:
        if k not in ("hpos", "var_covered", "var_fcov", "onHap"):
            assert set(np.nonzero(got[k][:pb.n_pairs] != want[k][:pb.n_pairs])[0].tolist()) | set(np.nonzero(exp[k][:pb.n_pairs] != want[k][:pb.n_pairs])[0].tolist()) <= set(rej.tolist()), k
    assert np.array_equal(got["hpos"], want["hpos"]) and np.array_equal(exp["hpos"], want["hpos"])
    diff = ps.first_difference(got, exp, pb, index)
    assert diff is not None and diff[2] in rej and diff[3] == "screened"                  # (the oracle's own status of that pair is DD_PAIR_NAN)
    elem = ps.element_pairs(pb)["hpos"][:pb.hpos_len]
    rl = np.diff(pb.a["read_seq_off"])
    w = int(np.searchsorted(pb.win_pair_off, hs[0], side="right")) - 1
    assert np.isin(elem, hs).sum() == int(rl[pb.a["win_read_off"][w]:pb.a["win_read_off"][w + 1]].sum())   # the hpos elements left out
    assert not np.isin(elem, rej).any()                                                 # (an empty read has none)


@functools.lru_cache(maxsize=None)
def faster_point(hl, L, mld):
    pb, index = ps.long_batch_for(hl, L, mld, wide=True, many="items")
    return pb, index, _oracle.batch(ps.params_for(mld), pb, nthreads=16, faster=True)


@pytest.mark.parametrize("hl,L,mld", FASTER_CASES)
def test_faster_long_batches(lib, hl, L, mld):
    """The --faster batches: more 16-pair items than the grid of the launch with the wide window can have workgroups; the oracle marks eight
    pairs DD_PAIR_NAN (the rejected window's two, the 1- and 2-bp reads on three haplotypes: "HapHash string too short") and the six hapSize
    pairs — compared as statuses; every other pair is computed."""
    pb, index, want = faster_point(hl, L, mld)
    n, i_n = ps.long_batch_for(hl, L, mld, wide=False, many="items")
    assert n.n_pairs == pb.n_pairs - 1 and all(np.array_equal(n.a[k], pb.a[k][:len(n.a[k])]) for k in n.a if not k.endswith("_table"))
    cls, _mx, n_bad = capi.screen_windows_ex(ps.params_for(mld), pb, capi.DD_OPT_LONG_WINDOWS_FASTER)
    assert (cls == capi.DD_WIN_LONG).sum() == pb.n_windows - 3 and n_bad == 1
    pairs, items = ps.long_pairs(pb, cls)
    assert items - 1 > ps.FASTER_LONG_WIDE_GRID_BOUND and (len(index["long.many"]) // 2 + 1) % 16
    st = want["status"][:pb.n_pairs]
    assert (st == capi.DD_PAIR_NAN).sum() == N_FASTER_NAN and (st[index["screened.rejected"]] == capi.DD_PAIR_NAN).all()
    rl = np.diff(pb.a["read_seq_off"])
    short = ps.element_pairs(pb)["onHap"][:pb.n_reads][(rl == 1) | (rl == 2)]           # (per read: its pair with the first haplotype)
    assert len(short) == 2 and (st[short] == capi.DD_PAIR_NAN).all()
    assert (st == capi.DD_PAIR_HAPSIZE).sum() == N_HAPSIZE and (st[index["screened.hapsize"]] == capi.DD_PAIR_HAPSIZE).all()
    assert (st == capi.DD_PAIR_OK).sum() == pb.n_pairs - N_FASTER_NAN - N_HAPSIZE
    assert np.isfinite(want["ll"][:pb.n_pairs][st == capi.DD_PAIR_OK]).all()


@pytest.mark.parametrize("mld,L", [pytest.param(mld, L, id="mld%d-L%d" % (mld, L)) for mld, L in ps.GRID])
def test_faster_kernel_batches(mld, L):
    """dd_faster_kernel's share of the matrix: the scenario batches of the main grid at FASTER_HAP_LENGTHS.  What its comparison leaves out:
    the oracle marks DD_PAIR_NAN exactly the pairs of a read of fewer than four bases ("HapHash string too short": the empty read of the
    rejected window, the 1- and 2-bp reads, at 30 bp the repeats' 2- and 3-bp reads) and DD_PAIR_HAPSIZE the five pairs of the 4-bp
    haplotype; those are compared as statuses, every other pair in every field."""
    lens = [hl for hl in ps.FASTER_HAP_LENGTHS if hl in ps.hap_lengths(mld)]
    assert lens == [hl for hl in ps.FASTER_HAP_LENGTHS if not (mld > 11 and hl > 574)] and len(lens) >= 4
    for hl in lens:
        pb, index = ps.batch_for(hl, L, mld)
        st = _oracle.batch(ps.params_for(mld), pb, nthreads=16, faster=True)["status"][:pb.n_pairs]
        hs = np.zeros(pb.n_pairs, bool)
        hs[index["screened.hapsize"]] = True
        rl = np.diff(pb.a["read_seq_off"])
        short = np.concatenate([np.tile(rl[pb.a["win_read_off"][w]:pb.a["win_read_off"][w + 1]] < 4, int(pb.a["win_hap_off"][w + 1] - pb.a["win_hap_off"][w]))
                                for w in range(pb.n_windows)])
        assert hs.sum() == N_HAPSIZE - 1 and np.array_equal(st == capi.DD_PAIR_HAPSIZE, hs), hl
        assert np.array_equal(st == capi.DD_PAIR_NAN, short & ~hs) and (st[~short & ~hs] == capi.DD_PAIR_OK).all(), hl
        assert (st == capi.DD_PAIR_NAN).sum() == (17 if hl == 30 else N_FASTER_NAN), hl
