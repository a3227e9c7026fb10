"""The scenario batches of tests/_path_scenarios.py reach the paths they are named after — shown on the oracle alone, for every grid point of
tests/test_gpu_path_matrix.py — and that grid reaches every (K, Dt, gbt, G) build dd_plan_info can return under the default environment.
No device: the oracle is the CPU restatement, the plan is host arithmetic (plan.cpp)."""
import ctypes as C
import functools

import numpy as np
import pytest

from dindel_tgi_amd import capi
from dindel_tgi_amd.batch import pack
from tests import _oracle
from tests import _path_scenarios as ps

CASES = [pytest.param(mld, L, id="mld%d-L%d" % (mld, L)) for mld, L in ps.GRID]


@functools.lru_cache(maxsize=None)
def point(mld, L, hl):
    """(PackedBatch, index, oracle arrays with mapUnmappedReads = 1) of one grid point, computed once for the module."""
    pb, index = ps.batch_for(hl, L, mld)
    return pb, index, _oracle.batch(ps.params_for(mld), pb, nthreads=16)


def points(mld, L):
    for hl in ps.hap_lengths(mld):
        yield (hl,) + point(mld, L, hl)


def test_grid_points_cover_both_sides_of_every_class_bound():
    assert ps.hap_lengths(5) == sorted({b for b in capi.HAP_CLASS_BOUNDS} | {b + 1 for b in capi.HAP_CLASS_BOUNDS[:-1]})
    assert max(ps.hap_lengths(15)) == 574 and min(ps.hap_lengths(15)) == 30


def test_builder_is_deterministic_and_keeps_the_shape():
    for hl, L, mld in ((94, 36, 11), (126, 100, 5), (255, 194, 10)):
        a, ia = ps.batch_for(hl, L, mld)
        b, ib = ps.batch_for(hl, L, mld)
        assert all(np.array_equal(a.a[k], b.a[k]) for k in a.a) and all(np.array_equal(ia[k], ib[k]) for k in ia)
        assert np.array_equal(a.hap_var_flank, b.hap_var_flank) and all(np.array_equal(a.mate[k], b.mate[k]) for k in a.mate)
        ws, _libs, index = ps.scenario_windows(hl, L, mld, np.random.default_rng(3))
        main = [w for w in ws if w.haps and len(w.haps[0]) == hl]
        assert len(main) >= 10 and all(hl - 3 <= len(h) <= hl for w in main for h in w.haps)       # the longest haplotype decides the build
        n_main = sum(len(w.reads) for w in main[:5])
        assert 60 <= n_main <= 100, n_main                                                           # redo, ends (two windows), mates, quals
        assert ("chunk.window" in index) == (hl <= 30 or 63 <= hl <= 94 or 127 <= hl <= 158)
        pb = pack(ws, libraries=_libs)
        for k in ps.FAMILIES:
            assert index[k].size == 0 or (0 <= index[k].min() and index[k].max() < pb.n_pairs), k
        assert all(index[k].size for k in ps.FAMILIES if k != "chunk")


@pytest.mark.parametrize("mld,L", CASES)
def test_redo_pairs_fall_below_the_bound_of_the_speculative_pass(mld, L):
    """At least 4 pairs with ll < -99 (both passes run) and at least 4 of the same window with ll > -99 (the pass without RO stands); two
    of the ordinary reads have the low ones' length, so both kinds also share a launch when reads are cut into length classes."""
    for hl, pb, index, want in points(mld, L):
        ll = want["ll"]
        assert (ll[index["redo"]] < -99).sum() >= 4, (hl, ll[index["redo"]])
        assert (ll[index["redo.ordinary"]] > -99).sum() >= 4, (hl, ll[index["redo.ordinary"]])
        rl = np.diff(pb.a["read_seq_off"])[:14]                                   # the redo window is the first: 6 low, 6 ordinary, 2 long ordinary
        assert (rl[:6] == max(L, ps.REDO_MIN_LEN)).all() and (rl[12:14] == max(L, ps.REDO_MIN_LEN)).all() and (rl[6:12] == L).all()


@pytest.mark.parametrize("mld,L", CASES)
def test_ends_reach_lo_ro_insertions_and_every_jump_length(mld, L):
    for hl, pb, index, want in points(mld, L):
        nind = want["numIndels"][index["ends.ladder"]]
        assert len(nind) == mld + 1 and (nind[:mld] == 1).all(), (hl, nind)        # one deletion each, lengths 1 .. maxLengthDel
        assert want["offHap"][index["ends.ladder"][mld]] == 1 or nind[mld] != 1     # maxLengthDel + 1: no single-jump explanation
        hp = want["hpos"][:pb.hpos_len]
        assert (hp == capi.DD_HPOS_LO).any() and (hp == capi.DD_HPOS_RO).any() and (hp <= capi.DD_HPOS_INS_KEY0).any(), hl
        rl = np.diff(pb.a["read_seq_off"])
        assert 1 in rl and 2 in rl
        assert 0xFFFFFFFF in pb.a["read_start"] and 3 in pb.a["read_start"] and (pb.a["read_flags"] & 1).any()


@pytest.mark.parametrize("mld,L", CASES)
def test_flags_take_both_values(mld, L):
    for hl, pb, index, want in points(mld, L):
        for k in ("var_covered", "var_fcov"):
            assert set(np.unique(want[k][:pb.var_cov_len]).tolist()) == {0, 1}, (hl, k)
        assert set(pb.hap_var_flank[2::3].tolist()) == {1, 2}


@pytest.mark.parametrize("mld,L", CASES)
def test_mate_prior_moves_the_pairs_with_a_usable_mate_only(mld, L):
    for hl, pb, index, want in points(mld, L):
        w = int(index["mates.window"][0])
        off = _oracle.batch(ps.params_for(mld, 0), pb, first_window=w, n_win=1)
        use, not_use = index["mates.usable"], index["mates.unusable"]
        assert len(use) + len(not_use) == 22 * 3 and len(use) >= 6 * 3
        assert (want["ll"][use] != off["ll"][use]).any(), hl
        assert np.array_equal(want["ll"][not_use], off["ll"][not_use]), hl
        fl = pb.a["read_flags"][pb.a["win_read_off"][w]:pb.a["win_read_off"][w] + 16] >> 1
        assert sorted(fl.tolist()) == list(range(16))                              # every combination of the four mate flags
        assert len(pb.mate["lib_p95"]) == 2 and set(pb.mate["read_lib"].tolist()) == {0, 1}


@pytest.mark.parametrize("mld,L", CASES)
def test_quals_fill_the_table_and_reach_both_offhap_outcomes(mld, L):
    for hl, pb, index, want in points(mld, L):
        assert pb.ctypes_batch().n_qual == 256 and len(np.unique(pb.a["qual_table"])) == 256, hl
        assert set(np.unique(want["offHap"][index["quals"]]).tolist()) == {0, 1}, hl
        mq = pb.a["mapq_table"]
        assert (mq > 1 - 1e-10).any() and 0.0 in mq and 1e-16 in mq              # past the Phred-100 cap, and the floor


@pytest.mark.parametrize("mld,L", CASES)
def test_bytes_and_ties_are_in_the_batch(mld, L):
    for hl, pb, index, want in points(mld, L):
        hb, rb = set(pb.a["hap_seq"].tobytes().decode()), set(pb.a["read_seq"].tobytes().decode())
        assert {"N", "R", "a", "n"} <= hb and {"N", "R", "n", "Y"} <= rb and len(hb - set("ACGTN")) <= 26
        haps = pb.a["hap_seq"].tobytes().decode()
        assert "AC" * 6 in haps and "CAG" * 4 in haps and "T" * 12 in haps and "A" * hl in haps and "NNN" in haps
        assert want["numMismatch"][index["bytes"]].any()


@pytest.mark.parametrize("mld,L", CASES)
def test_screened_windows_ride_along(lib, mld, L):
    for hl, pb, index, want in points(mld, L):
        skip = np.zeros(pb.n_windows, np.uint8)
        mx = (C.c_int32 * 2)()
        assert lib.dd_screen_windows(C.byref(pb.ctypes_batch()), skip.ctypes.data_as(capi.c_u8p), C.byref(mx)) == 1
        rej = index["screened.rejected"]
        w = int(np.nonzero(skip)[0][0])
        assert rej.tolist() == list(range(int(pb.win_pair_off[w]), int(pb.win_pair_off[w + 1]))) and mx[0] == hl
        H, R = np.diff(pb.a["win_hap_off"]), np.diff(pb.a["win_read_off"])
        assert ((H > 0) & (R == 0)).any() and ((H == 0) & (R > 0)).any()
        st = want["status"][:pb.n_pairs]
        hs = index["screened.hapsize"]                                             # (every grid point has maxLengthDel >= 5)
        assert len(hs) == 5 and (st[hs] == capi.DD_PAIR_HAPSIZE).all()
        rest = np.ones(pb.n_pairs, bool)
        rest[rej] = False
        rest[hs] = False
        assert (st[rest] == capi.DD_PAIR_OK).all(), hl


@pytest.mark.parametrize("mld,L", CASES)
def test_chunk_window_orders_two_chunks_and_pairs_unequal_reads(lib, mld, L):
    """More than DD_HALF_CHUNK (256) reads in one window of a half-wave class, of three lengths.  Read off the kernel's sort key
    (hmm_kernel.hip, the G = 2 ordering: key = ((L - 1) >> 3) << 11 | bMid term, ties by read index; a wavefront takes two consecutive
    ranks, and the read split hands out whole units of two ranks): the order within a length bucket depends on bMid, the bucket
    boundaries do not, so a chunk pairs reads of unequal length exactly when a bucket's cumulative count is odd.  That is checked here for
    both chunks; that the window's launch is a G = 2 build comes from the plan (the D = 32 build of maxLengthDel > 11 has whole wavefronts only).  Which wavefront ran which two reads is not observable
    from the results (they do not depend on the order): the GPU matrix asserts from the launch log that the launch took place."""
    seen = 0
    for hl, pb, index, want in points(mld, L):
        G = next(c[1] for c in capi.HAP_CLASSES if hl <= c[0])
        assert ("chunk.window" in index) == (G == 2)
        if "chunk.window" not in index:
            continue
        seen += 1
        w = int(index["chunk.window"][0])
        r0, r1 = int(pb.a["win_read_off"][w]), int(pb.a["win_read_off"][w + 1])
        rl = np.diff(pb.a["read_seq_off"])[r0:r1 + 0]
        assert r1 - r0 > 256 and sorted(set(rl.tolist())) == list(ps.CHUNK_LENS)
        for c0 in range(0, r1 - r0, 256):
            by_rank = np.sort((rl[c0:c0 + 256] - 1) >> 3, kind="stable")           # buckets in rank order
            pairs = by_rank[:len(by_rank) // 2 * 2].reshape(-1, 2)
            assert (pairs[:, 0] != pairs[:, 1]).any(), (hl, c0)
        p = ps.params_for(mld)
        cls = np.searchsorted(capi.HAP_CLASS_BOUNDS, hl)
        assert mld > 11 or any(b[3] == 2 and b[4] == cls and b[5] >= max(ps.CHUNK_LENS) and b[5] <= 160 for b in ps.planned_builds(lib, p, pb)), hl
    assert seen == 5                                         # 30, 63, 94, 127 and 158 bp


def test_grid_reaches_every_build_the_plan_can_select(lib):
    """dd_plan_info over both sides of every class bound x read lengths 1 .. 1024 x maxLengthDel 0 .. 31 at the batches' table size: the
    distinct (K, Dt, gbt, G) under the default environment — and every one of them is planned for some launch of some grid point."""
    out = (C.c_int32 * 10)()
    can = set()
    lens = list(range(1, 400)) + list(range(400, 1025, 8)) + [1024]
    for mld in range(32):
        p = ps.params_for(mld, 0)
        for hl in sorted({1} | {h for b in capi.HAP_CLASS_BOUNDS for h in (b, b + 1) if h <= capi.DD_MAX_HAP_LEN}):
            for rl in lens:
                if lib.dd_plan_info(C.byref(p), hl, rl, 256, 50, 100, C.byref(out)) == 0:
                    can.add((out[0], out[1], out[2], out[8]))
    assert len(can) >= 61 and {k[1] for k in can} == {6, 11, 12, 32} and {(k[0], k[3]) for k in can if k[3] == 2} == {(1, 2), (3, 2), (5, 2)}
    reached = set()
    for mld, L in ps.GRID:
        for hl, pb, index, want in points(mld, L):
            reached |= {b[:4] for b in ps.planned_builds(lib, ps.params_for(mld), pb)}
    assert not can - reached, sorted(can - reached)
