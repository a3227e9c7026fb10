"""Which elements of the result arrays a likelihood call owns, and the buffers that show it (helper; no tests in here).

A parity test compares values; it cannot tell an element the kernels wrote from one that already held the right value — a zeroed torch
tensor, or the results the last call left in the host path's arena.  Here every result buffer starts out as bytes 0x5A (BODY_BYTE) between
guards of 0xA5 (GUARD_BYTE), and after the call

  every element the library is contracted to write (must_write) is bit-equal to its expected value — none of which has the poison's bit
  pattern (tests/test_output_ownership_cpu.py), so it was written;
  every other element still holds the poison in every byte, and so does nothing around the arrays (the guards).

  Guarded        the host arrays in page-locked memory (written in place), GUARD bytes longer at each end
  GuardedDevice  the same around the tensors of a DeviceBatch
  must_write     the contract, from include/dindel_hmm.h and the kernels' stores (no GPU run went into it)
  assert_owned   the check, reporting array, element, pair and scenario family like _path_scenarios.first_difference

The contract (dd_result in include/dindel_hmm.h:64-71 and :165-185; the stores named are the only ones for such a pair):

  DD_PAIR_OK             every per-pair value, the pair's hpos, var_covered, and var_fcov when the batch has hap_var_flank
                         (hmm_kernel.hip:1269-1447, faster_kernel.hip:136-161 and :301-310, faster_pair_end.inc)
  DD_PAIR_NAN / _LLPOS   main model: as DD_PAIR_OK — the status is found from the finished ll (hmm_kernel.hip:1400-1402)
                         --faster: a read shorter than the 4-mer is finished ahead of the sweeps (faster_kernel.hip:136-161): status,
                         ll = 0, offHapHMQ = 1, zero in the nine values this model leaves at MLAlignment's defaults and in offHap, both
                         coverage flags 0; no firstBase, lastBase, hpos
  DD_PAIR_HAPSIZE        main model: status, ll = 0, both coverage flags 0 (hmm_kernel.hip:576-589 mark_hapsize), nothing else
                         --faster: as its DD_PAIR_NAN (the same lines)
  DD_PAIR_UNSUPPORTED    status, ll = 0, offHap = offHapHMQ = 1 (hmm_kernel.hip:183-189 mark_unsupported, faster_kernel.hip:73-82)
  onHap                  every read of every window the launch covers, windows without haplotypes included (hmm_kernel.hip:1459-1481;
                         host_path.cpp:148 for a batch without pairs): 0 for a read whose pairs are all DD_PAIR_HAPSIZE or _UNSUPPORTED
"""
import contextlib
import ctypes as C
import functools
import os

import numpy as np

from dindel_tgi_amd import capi
from dindel_tgi_amd.batch import RESULT_DTYPES, result_lengths
from tests import _path_scenarios as ps

GUARD = 256
GUARD_BYTE, BODY_BYTE = 0xA5, 0x5A
PER_ELEMENT = ("hpos", "var_covered", "var_fcov", "onHap")
PAIR_KEYS = [k for k, _t in capi.RESULT_FIELDS if k not in PER_ELEMENT]
# the --faster model leaves these at MLAlignment's defaults; offHapHMQ besides is 1 for a pair the reference throws for
FASTER_DEFAULTS = ("llOn", "llOff", "mLogBQ", "offHap", "numIndels", "numMismatch", "nBQT", "nmmBQT", "nMMLeft", "nMMRight")


class Guarded:
    """Every dd_result array in page-locked memory (dd_host_alloc), GUARD bytes longer at each end; the dd_result holds the interior
    pointers.  Guards and body carry different sentinels.  pageable=True: the same layout in numpy's own memory (no device needed: the
    library then copies the results back instead of writing them in place); flip=(array, byte offset into the raw buffer): that byte is
    inverted after the fill, as a stray store would leave it."""

    def __init__(self, lib, pb, pageable=False, flip=None):
        self.lib, self.n, self.raw, self.ptrs = lib, result_lengths(pb), {}, []
        self.res = capi.dd_result()
        for k, typ in capi.RESULT_FIELDS:
            nbytes = max(self.n[k], 1) * np.dtype(RESULT_DTYPES[k]).itemsize
            if pageable:
                self.raw[k] = np.zeros(nbytes + 2 * GUARD, np.uint8)
                ptr = self.raw[k].ctypes.data
            else:
                ptr = lib.dd_host_alloc(nbytes + 2 * GUARD)
                assert ptr, k
                self.ptrs.append(ptr)
                self.raw[k] = np.frombuffer((C.c_char * (nbytes + 2 * GUARD)).from_address(ptr), dtype=np.uint8)
            self.raw[k][...] = GUARD_BYTE
            self.raw[k][GUARD:GUARD + nbytes] = BODY_BYTE
            setattr(self.res, k, C.cast(C.c_void_p(ptr + GUARD), typ))
        if flip is not None:
            self.raw[flip[0]][flip[1]] ^= 0xFF

    def body(self, k):
        return self.raw[k][GUARD:len(self.raw[k]) - GUARD].view(RESULT_DTYPES[k])

    def arrays(self):
        """Copies of the bodies, as alloc_result returns the arrays."""
        return {k: self.body(k).copy() for k, _t in capi.RESULT_FIELDS}

    def check_guards(self, where):
        for k, _typ in capi.RESULT_FIELDS:
            raw = self.raw[k]
            assert (raw[:GUARD] == GUARD_BYTE).all(), "%s: %s: the guard in front of the array was written at byte %d" % (
                where, k, int(np.nonzero(raw[:GUARD] != GUARD_BYTE)[0][0]) - GUARD)
            assert (raw[-GUARD:] == GUARD_BYTE).all(), "%s: %s: the guard behind the array was written at byte +%d" % (
                where, k, int(np.nonzero(raw[-GUARD:] != GUARD_BYTE)[0][0]))

    def check(self, plain, pb, index, where):
        """Both guards untouched; the body byte-equal to the pageable run `plain` — but for elements that still hold the body sentinel, and
        those only where the pageable run shows that the library does not write them: elements of a pair whose status there is not
        DD_PAIR_OK (the rejected window's pairs, of which the library defines five values; the hpos of a hapSize-error pair), or of no pair
        (the onHap of a read in a window without haplotypes).  -> the number of such elements per array."""
        status = plain["status"][:pb.n_pairs]
        elem = ps.element_pairs(pb)
        left = {}
        self.check_guards(where)
        for k, _typ in capi.RESULT_FIELDS:
            n, size = self.n[k], np.dtype(RESULT_DTYPES[k]).itemsize
            if n == 0:
                continue
            mine = self.body(k)[:n].view(np.uint8).reshape(n, size)
            ref = np.ascontiguousarray(plain[k][:n]).view(np.uint8).reshape(n, size)
            differ = np.nonzero((mine != ref).any(axis=1))[0]
            if differ.size == 0:
                continue
            pair = elem[k][differ] if k in PER_ELEMENT else differ
            sentinel = (mine[differ] == BODY_BYTE).all(axis=1)
            unwritten = (pair < 0) | (status[np.maximum(pair, 0)] != capi.DD_PAIR_OK)
            bad = np.nonzero(~(sentinel & unwritten))[0]
            assert bad.size == 0, "%s: %s[%d] (pair %d, family %s) is %r in place, %r through the copy" % (
                where, k, int(differ[bad[0]]), int(pair[bad[0]]), ps.family_of(int(pair[bad[0]]), index), self.body(k)[int(differ[bad[0]])], plain[k][int(differ[bad[0]])])
            left[k] = int(differ.size)
        return left

    def release(self):
        self.raw.clear()
        while self.ptrs:
            self.lib.dd_host_free(self.ptrs.pop())


class GuardedDevice:
    """The result tensors of a DeviceBatch replaced by views into buffers GUARD bytes longer at each end: dev.out[k] is a typed view of the
    body, dev.dr.<k> its address (256-byte aligned, as torch's own allocations are).  Guards and body carry different sentinels."""

    def __init__(self, dev, body_byte=BODY_BYTE):
        import torch
        from dindel_tgi_amd.device import _TORCH_DT
        self.dev, self.raw = dev, {}
        for k, _typ in capi.RESULT_FIELDS:
            dt = np.dtype(RESULT_DTYPES[k])
            nbytes = max(dev._n[k], 1) * dt.itemsize
            raw = torch.empty(nbytes + 2 * GUARD, dtype=torch.uint8, device=dev.device)
            assert raw.data_ptr() % 256 == 0 and GUARD % 256 == 0, k
            self.raw[k] = raw
            dev.out[k] = raw[GUARD:GUARD + nbytes].view(_TORCH_DT[dt])
            assert dev.out[k].data_ptr() == raw.data_ptr() + GUARD
            setattr(dev.dr, k, dev.out[k].data_ptr())
        self.fill(body_byte)

    def fill(self, body_byte=BODY_BYTE):
        import torch
        for raw in self.raw.values():
            raw.fill_(GUARD_BYTE)
            raw[GUARD:len(raw) - GUARD].fill_(body_byte)
        torch.cuda.synchronize(self.dev.device)

    def check(self, where):
        """Both guards of every array untouched (one copy back)."""
        import torch
        torch.cuda.synchronize(self.dev.device)
        keys = [k for k, _typ in capi.RESULT_FIELDS]
        g = torch.cat([t for k in keys for t in (self.raw[k][:GUARD], self.raw[k][-GUARD:])]).cpu().numpy().reshape(len(keys), 2, GUARD)
        for i, k in enumerate(keys):
            for side, name in ((0, "in front of"), (1, "behind")):
                bad = np.nonzero(g[i, side] != GUARD_BYTE)[0]
                assert bad.size == 0, "%s: %s: the guard %s the array was written at byte %+d" % (
                    where, k, name, int(bad[0]) - (GUARD if side == 0 else 0))


def alloc_poisoned(pb):
    """batch.alloc_result with the poison in every byte of every array (its fill= is a value per element)."""
    from dindel_tgi_amd.batch import alloc_result
    arrs, res = alloc_result(pb, fill=BODY_BYTE)
    for a in arrs.values():
        a.view(np.uint8)[...] = BODY_BYTE
    return arrs, res


@contextlib.contextmanager
def poisoned_arena():
    """DD_POISON_OUTPUTS=1 around a host-pointer call: the arena's output region starts out as the poison, not as the last call's
    results.  The environment is put back as it was."""
    saved = os.environ.get("DD_POISON_OUTPUTS")
    os.environ["DD_POISON_OUTPUTS"] = "1"
    try:
        yield
    finally:
        if saved is None:
            os.environ.pop("DD_POISON_OUTPUTS", None)
        else:
            os.environ["DD_POISON_OUTPUTS"] = saved


class Ownership:
    """must_write's answer.  write[k]: the elements of array k the library is contracted to write; expected[k]: their values — the oracle's,
    or the header's where the library defines another (a copy: the oracle's arrays stay as they are); status: the expected status per pair;
    index: the scenario families, for the report."""

    def __init__(self, write, expected, index):
        self.write, self.expected, self.index = write, expected, index
        self.status = expected["status"]


def unsupported_pairs(pb):
    """The pairs of the windows dd_screen_windows rejects (host arithmetic: no device), as a mask over the pairs."""
    b = pb.ctypes_batch()
    skip = np.zeros(max(pb.n_windows, 1), np.uint8)
    mx = (C.c_int32 * 2)()
    assert capi.load().dd_screen_windows(C.byref(b), skip.ctypes.data_as(capi.c_u8p), C.byref(mx)) >= 0, capi.last_error()
    out = np.zeros(pb.n_pairs, bool)
    for w in np.nonzero(skip[:pb.n_windows])[0]:
        out[int(pb.win_pair_off[w]):int(pb.win_pair_off[w + 1])] = True
    return out


def must_write(pb, want, index=None, faster=False):
    """-> Ownership: per result array, the elements a likelihood call on pb is contracted to write, and their values (`want`: the oracle's
    arrays of the same model).  The module docstring has the contract and where it was read."""
    n = result_lengths(pb)
    P = pb.n_pairs
    OK, HAPSIZE, NAN, UNSUPPORTED = capi.DD_PAIR_OK, capi.DD_PAIR_HAPSIZE, capi.DD_PAIR_NAN, capi.DD_PAIR_UNSUPPORTED
    exp = {k: np.array(want[k][:max(n[k], 1)], copy=True) for k, _t in capi.RESULT_FIELDS}
    unsup = unsupported_pairs(pb)
    exp["status"][:P][unsup] = UNSUPPORTED
    st = exp["status"][:P]
    hapsize = st == HAPSIZE
    # pairs the model works out to the end / finishes ahead of the sweeps with defined values
    computed = (st == OK) if faster else ~(hapsize | unsup)
    thrown = ~(computed | unsup) if faster else np.zeros(P, bool)
    assert not faster or np.isin(st, (OK, HAPSIZE, NAN, UNSUPPORTED)).all()

    write = {}
    for k in PAIR_KEYS:
        if k in ("status", "ll"):
            m = np.ones(P, bool)
        elif k in ("offHap", "offHapHMQ"):
            m = computed | unsup | thrown
        elif k in ("firstBase", "lastBase"):
            m = computed
        else:
            m = computed | thrown
        write[k] = m
    exp["ll"][:P][unsup | hapsize | thrown] = 0.0
    exp["offHap"][:P][unsup] = 1
    exp["offHapHMQ"][:P][unsup | thrown] = 1
    for k in FASTER_DEFAULTS:
        exp[k][:P][thrown] = 0

    elem = ps.element_pairs(pb)
    flanks = pb.hap_var_flank is not None and len(pb.hap_var_flank) > 0
    of = {k: elem[k][:n[k]] for k in PER_ELEMENT}
    write["hpos"] = computed[of["hpos"]]
    failed = hapsize | thrown
    write["var_covered"] = ~unsup[of["var_covered"]]
    write["var_fcov"] = (~unsup if flanks else failed)[of["var_fcov"]]
    for k in ("var_covered", "var_fcov"):
        exp[k][:n[k]][failed[of[k]]] = 0
    write["onHap"] = np.ones(n["onHap"], bool)
    # a read is on a haplotype iff one of its computed pairs says so: never through a rejected window's pairs
    reads = of["onHap"]
    exp["onHap"][:n["onHap"]][(reads >= 0) & unsup[np.maximum(reads, 0)]] = 0
    exp["onHap"][:n["onHap"]][reads < 0] = 0
    for k in write:
        assert write[k].shape == (n[k],), k
    return Ownership(write, exp, index)


def _pair_of(k, e, elem):
    return int(elem[k][e]) if k in PER_ELEMENT else int(e)


def assert_owned(got, want, pb, mask, where):
    """Every element of mask.write is bit-equal to its expected value (mask.expected: `want`, the oracle's arrays, but for the values the
    library defines itself), and every other element still holds BODY_BYTE in every byte.  The failure with the lowest pair index is
    reported: array, element, pair, scenario family, and which of the two it is."""
    n = result_lengths(pb)
    elem = ps.element_pairs(pb)
    best = None
    for k, _typ in capi.RESULT_FIELDS:
        if n[k] == 0:
            continue
        size = np.dtype(RESULT_DTYPES[k]).itemsize
        if k in PAIR_KEYS:           # the expected values are the oracle's wherever the pair was computed: the mask belongs to `want`
            ok = mask.write[k] & (mask.status[:n[k]] == capi.DD_PAIR_OK)
            assert np.array_equal(np.asarray(want[k][:n[k]])[ok], mask.expected[k][:n[k]][ok]), "%s: %s: the mask was not made from these arrays" % (where, k)
        g =np.ascontiguousarray(got[k][:n[k]]).view(np.uint8).reshape(n[k], size)
        e = np.ascontiguousarray(mask.expected[k][:n[k]]).view(np.uint8).reshape(n[k], size)
        m = mask.write[k]
        bad = np.nonzero((m & (g != e).any(axis=1)) | (~m & (g != BODY_BYTE).any(axis=1)))[0]
        if bad.size == 0:
            continue
        pairs = elem[k][bad] if k in PER_ELEMENT else bad
        i = int(np.argmin(pairs))
        if best is None or int(pairs[i]) < best[2]:
            best = (k, int(bad[i]), int(pairs[i]))
    if best is None:
        return
    k, e, pair = best
    value = np.ascontiguousarray(got[k][:n[k]])[e]
    poison = bool((np.ascontiguousarray(got[k][:n[k]]).view(np.uint8).reshape(n[k], -1)[e] == BODY_BYTE).all())
    status = int(mask.status[pair]) if pair >= 0 else -1
    family = ps.family_of(pair, mask.index) if mask.index is not None and pair >= 0 else "none"
    if mask.write[k][e]:
        what = "still holds the poison: it was never written" if poison else "is %r, expected %r" % (value, mask.expected[k][e])
    else:
        what = "is %r: written, though the library does not own it (status %d)" % (value, status)
    raise AssertionError("%s: family %s, pair %d (status %d): %s[%d] %s" % (where, family, pair, status, k, e, what))


def edges_batch(mld=5):
    """-> (PackedBatch, index map, params): six hand-built windows whose last array elements border the rear guard.
      1  two haplotypes, no read          2  three reads, no haplotype       3  one haplotype, one 1-bp read (--faster: DD_PAIR_NAN)
      4  haplotypes of 40 and 130 bp (two launch classes write one window's arrays), read bases odd in total (the next window's hpos
         starts at an odd int16 offset)    5  haplotypes carrying 0, 1 and 3 variants    6  a haplotype shorter than maxLengthDel"""
    from dindel_tgi_amd.batch import Window, ReadRec, pack
    rng = np.random.default_rng(20240607)
    S = ps.HAP_START
    h40, h130, h60 = ps.rnd(rng, 40), ps.rnd(rng, 130), ps.rnd(rng, 60)
    r4 = ps.spread_reads(rng, h130, 3, 36) + ps.spread_reads(rng, h40, 2, 30) + [ps.ReadRec(h130[50:87], [ps.Q20] * 37, ps.MQ, S + 50)]
    assert sum(len(r.seq) for r in r4) % 2 == 1
    haps5 = [h60, h60[:30] + h60[32:], h60[:20] + "AC" + h60[20:]]
    ws = [Window(S, [h40, h40[:20] + h40[21:]], []),
          Window(S, [], ps.spread_reads(rng, h40, 3, 30)),
          Window(S, [h40], [ReadRec(h40[10:11], [ps.Q20], ps.MQ, S + 10)]),
          Window(S, [h40, h130], r4, hap_vars=[[(20, 21)], [(64, 66)]], hap_var_flanks=[[(19, 22, 1)], [(63, 67, 2)]]),
          Window(S, haps5, ps.spread_reads(rng, h60, 5, 36), hap_vars=[[], [(30, 31)], [(20, 22), (1, 2), (40, 40)]],
                 hap_var_flanks=[[], [(29, 32, 1)], [(19, 23, 2), (0, 3, 1), (39, 41, 0)]]),
          Window(S, [h60, "ACGT"[:mld - 1]], ps.spread_reads(rng, h60, 4, 30), hap_vars=[[(10, 11)], [(1, 2)]],
                 hap_var_flanks=[[(9, 12, 1)], [(0, 3, 2)]])]
    pb = pack(ws)
    p = ps.params_for(mld, 0)
    return pb, {"edges": np.arange(pb.n_pairs, dtype=np.int64)}, p


SCENARIO_SHAPES = ((30, 36, 5), (126, 36, 5), (127, 36, 5), (159, 36, 5), (254, 100, 11))


def batches():
    """The batches of tests/test_gpu_output_ownership.py and tests/test_output_ownership_cpu.py: name -> builder of (pb, index, params)."""
    out = {"hap%d-L%d-mld%d" % s: (lambda s=s: ps.batch_for(*s) + (ps.params_for(s[2], 1),)) for s in SCENARIO_SHAPES}
    out["edges"] = edges_batch
    return out


@functools.lru_cache(maxsize=None)
def case(name, faster):
    """(PackedBatch, index, params, oracle arrays, Ownership) of a batch and a model: one oracle run, shared and left unchanged."""
    from tests import _oracle
    pb, index, p = batches()[name]()
    want = _oracle.batch(p, pb, nthreads=16, faster=faster)
    for a in want.values():
        a.setflags(write=False)
    return pb, index, p, want, must_write(pb, want, index, faster=faster)
