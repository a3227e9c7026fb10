"""The harness of tests/test_gpu_output_ownership.py, shown on the oracle alone: no device.

For every batch of that module and both models: no element the library must write has the poison's bit pattern in the expected arrays (so
"bit-equal to the expected value" proves a store); what the contract leaves out of the mask stays small; and assert_owned fails — naming the
array — for one unwritten element of any array, for one stray store into an element the library does not own, and Guarded.check_guards
for one changed guard byte.  That is what makes a pass on the GPU mean something."""
import os

import numpy as np
import pytest

from dindel_tgi_amd import capi
from dindel_tgi_amd.batch import result_lengths
from tests import _output_ownership as oo
from tests import _path_scenarios as ps

BATCHES = oo.batches()
CASES = [pytest.param(name, faster, id="%s-%s" % (name, "faster" if faster else "main")) for name in BATCHES for faster in (False, True)]
MODES = ({}, {"DD_DYNAMIC": "1", "DD_FORCE_GBT": "0"}, {"DD_FORCE_GBT": "1"}, {"DD_NO_HALF": "1"},
         {"DD_NO_HALF": "1", "DD_DYNAMIC": "1", "DD_FORCE_GBT": "0"})          # tests/test_gpu_persistent_rounds.MODES (a GPU module: not imported here)


case = oo.case


def poisoned(a):
    """Per element: every byte is the poison's."""
    a = np.ascontiguousarray(a)
    return (a.view(np.uint8).reshape(len(a), -1) == oo.BODY_BYTE).all(axis=1)


@pytest.mark.parametrize("name,faster", CASES)
def test_no_owned_value_looks_like_the_poison(name, faster):
    pb, _index, _p, want, own = case(name, faster)
    n = result_lengths(pb)
    for k, _t in capi.RESULT_FIELDS:
        assert own.write[k].dtype == bool and own.write[k].shape == (n[k],), k
        hit = np.nonzero(poisoned(own.expected[k][:n[k]]) & own.write[k])[0]
        assert hit.size == 0, "%s[%d] = %r has the poison's bit pattern: change the batch's seed" % (k, int(hit[0]), own.expected[k][hit[0]])
        assert not poisoned(np.asarray(want[k][:n[k]])).any(), k                               # (nor does any value of the oracle's)


@pytest.mark.parametrize("name,faster", CASES)
def test_the_mask_is_the_oracle_but_for_what_the_header_defines(name, faster):
    """Where must_write's expected value is not the oracle's: only pairs that were not computed (their status says so), the onHap of a
    rejected window's reads — and, in the --faster model, nothing of a DD_PAIR_OK pair."""
    pb, index, _p, want, own = case(name, faster)
    n = result_lengths(pb)
    elem = ps.element_pairs(pb)
    st = own.status[:pb.n_pairs]
    for k, _t in capi.RESULT_FIELDS:
        changed = np.nonzero(np.asarray(want[k][:n[k]]) != own.expected[k][:n[k]])[0]
        pairs = elem[k][changed] if k in oo.PER_ELEMENT else changed
        assert (pairs >= 0).all() and (st[pairs] != capi.DD_PAIR_OK).all(), (k, changed[:5])
    if "screened.rejected" in index:
        assert np.array_equal(np.nonzero(st == capi.DD_PAIR_UNSUPPORTED)[0], np.sort(index["screened.rejected"]))
    oo.assert_owned(own.expected, want, pb, all_written(own, pb), "expected against itself")    # (with every element in the mask it only compares)


def all_written(own, pb):
    """own with every element in the mask: assert_owned then only compares."""
    n = result_lengths(pb)
    return oo.Ownership({k: np.ones(n[k], bool) for k in own.write}, own.expected, own.index)


@pytest.mark.parametrize("name,faster", CASES)
def test_what_the_mask_leaves_out_is_small(name, faster):
    pb, _index, _p, _want, own = case(name, faster)
    st = own.status[:pb.n_pairs]
    counts = {s: int((st == s).sum()) for s in range(5)}
    left = int((~own.write["hpos"]).sum())
    print("ownership %s %s: %d pairs, per status %r; hpos outside the mask %d of %d" % (name, "faster" if faster else "main", pb.n_pairs, counts, left, pb.hpos_len))
    if name == "edges":
        # window 3: 1 pair (a 1-bp read); window 4: 2 x 6; window 5: 3 x 5; window 6: 2 x 4, the 4-bp haplotype's four fail
        assert pb.n_pairs == 36 and pb.n_windows == 6 and pb.n_reads == 19
        want = {capi.DD_PAIR_OK: 31, capi.DD_PAIR_HAPSIZE: 4, capi.DD_PAIR_NAN: 1} if faster else {capi.DD_PAIR_OK: 32, capi.DD_PAIR_HAPSIZE: 4}
        assert {s: c for s, c in counts.items() if c} == want, counts
        assert pb.win_hpos_off[4] % 2 == 1                                                     # the next window's hpos starts at an odd offset
        return
    assert 14 <= pb.n_windows <= 15 and pb.n_pairs <= 950, (pb.n_windows, pb.n_pairs)
    assert pb.n_pairs - counts[capi.DD_PAIR_OK] <= 0.05 * pb.n_pairs, counts
    assert left <= 0.01 * pb.hpos_len, (left, pb.hpos_len)
    assert counts[capi.DD_PAIR_HAPSIZE] > 0 and counts[capi.DD_PAIR_UNSUPPORTED] > 0, counts     # the batch holds what the contract is about


@pytest.mark.parametrize("name,faster", CASES)
def test_one_unwritten_element_of_any_array_is_found(name, faster):
    """The oracle's own arrays pass; with the poison in one owned element — first, last, one in the middle — of each array in turn,
    assert_owned raises and names the array and the element."""
    pb, _index, _p, want, own = case(name, faster)
    n = result_lengths(pb)
    clean = {k: own.expected[k].copy() for k in own.expected}
    for k in clean:                                                        # what a correct library leaves behind
        clean[k][:n[k]].view(np.uint8).reshape(n[k], -1)[~own.write[k]] = oo.BODY_BYTE
    oo.assert_owned(clean, want, pb, own, "untouched")
    tried = 0
    for k, _t in capi.RESULT_FIELDS:
        owned = np.nonzero(own.write[k])[0]
        assert owned.size >= 3, k
        for e in (int(owned[0]), int(owned[-1]), int(owned[owned.size // 2])):
            got = dict(clean)
            got[k] = clean[k].copy()
            got[k][:n[k]].view(np.uint8).reshape(n[k], -1)[e] = oo.BODY_BYTE
            with pytest.raises(AssertionError, match=r"%s\[%d\] still holds the poison" % (k, e)):
                oo.assert_owned(got, want, pb, own, "mutated")
            tried += 1
    assert tried == 3 * len(capi.RESULT_FIELDS) == 57


@pytest.mark.parametrize("name,faster", CASES)
def test_one_stray_store_is_found(name, faster):
    """A plausible value in an element the library does not own: assert_owned raises for it, in every array that has such an element; a
    wrong value in an owned element likewise."""
    pb, _index, _p, want, own = case(name, faster)
    n = result_lengths(pb)
    clean = {k: own.expected[k].copy() for k in own.expected}
    for k in clean:
        clean[k][:n[k]].view(np.uint8).reshape(n[k], -1)[~own.write[k]] = oo.BODY_BYTE
    arrays = 0
    for k, _t in capi.RESULT_FIELDS:
        free = np.nonzero(~own.write[k])[0]
        if free.size:
            arrays += 1
            got = dict(clean)
            got[k] = clean[k].copy()
            got[k][int(free[-1])] = 0
            with pytest.raises(AssertionError, match=r"%s\[%d\] is .*does not own" % (k, int(free[-1]))):
                oo.assert_owned(got, want, pb, own, "stray")
        e = int(np.nonzero(own.write[k])[0][-1])
        got = dict(clean)
        got[k] = clean[k].copy()
        got[k][e] = got[k][e] + 1
        with pytest.raises(AssertionError, match=r"%s\[%d\] is " % (k, e)):
            oo.assert_owned(got, want, pb, own, "wrong")
    assert arrays >= (14 if not faster else 3), arrays        # main model: every per-pair array but ll and status, and hpos


def test_a_changed_guard_byte_is_found():
    pb, _index, _p = BATCHES["edges"]()
    lib = capi.load()
    g = oo.Guarded(lib, pb, pageable=True)
    g.check_guards("untouched")
    assert all((g.body(k).view(np.uint8) == oo.BODY_BYTE).all() for k, _t in capi.RESULT_FIELDS)
    assert all(g.raw[k].ctypes.data + oo.GUARD == np.ctypeslib.as_array(getattr(g.res, k), (1,)).ctypes.data for k, _t in capi.RESULT_FIELDS)
    n = result_lengths(pb)
    for k, off, text in (("hpos", oo.GUARD - 1, "in front of"), ("status", oo.GUARD + n["status"] * 4, "behind"),
                         ("var_fcov", oo.GUARD + max(n["var_fcov"], 1) + oo.GUARD - 1, "behind"), ("ll", 0, "in front of")):
        bad = oo.Guarded(lib, pb, pageable=True, flip=(k, off))
        with pytest.raises(AssertionError, match="%s: the guard %s the array" % (k, text)):
            bad.check_guards("flipped")


@pytest.mark.parametrize("name", list(BATCHES))
def test_the_modes_select_more_than_one_kernel(name):
    """Host arithmetic only (ps.planned_builds): over the five launch modes the plan picks at least two distinct builds for every batch,
    so the poisoned arena of the host-path leg is not checked on one kernel alone."""
    pb, _index, p = BATCHES[name]()
    keys = ("DD_DYNAMIC", "DD_FORCE_GBT", "DD_NO_HALF")
    saved = {k: os.environ.pop(k, None) for k in keys}
    try:
        builds = set()
        for env in MODES:
            for k in keys:
                os.environ.pop(k, None)
            os.environ.update(env)
            builds |= {b[:4] for b in ps.planned_builds(capi.load(), p, pb)}
    finally:
        for k in keys:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    assert len(builds) >= 2, builds
