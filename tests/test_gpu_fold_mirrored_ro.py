"""The right->middle pass with RO folded into the generic candidate code in BOTH slots of its lane (hmm_kernel.hip, FOLD / mirRO).

At K = 2 the RO state of a haplotype of even length sits in its lane's last slot and has been folded since round 3; for odd lengths it
sits in the first slot and now rides there as well, with the lane's dead second slot as a copy of it ("mirrored"), as long as two more
positions are free in front of LO's idle position: odd Hs <= 121.  Hs = 123 keeps the one-lane block.  Every window here holds all three
kinds (117..123 bp), one window ends in a homopolymer / short-repeat tail (exact ties at RO), and the reads make the MAP path enter RO,
stay there and pass through the inserted state numS+RO; some reads are random sequence, some 12 bp long.

Checked for the three K = 2 builds that carry the fold (D = 6 with LDS and with scratch back-pointers, D = 11 with LDS back-pointers) and
for a launch whose workgroups take a second and a third item: every result field bit-equal to the oracle, for every pair, and bit-equal
between the folded launch and the same batch under DD_NO_FOLD=1 (the one-lane blocks)."""
import os

import numpy as np
import pytest

from dindel_tgi_amd import capi
from dindel_tgi_amd.batch import RESULT_DTYPES, ReadRec, Window, pack, result_lengths
from tests import _oracle
from tests.test_gpu_parity import run_host_api

pytestmark = pytest.mark.gpu

LENGTHS = (117, 118, 119, 120, 121, 122, 123, 121)       # per window: both parities, the largest mirrored (121) and plainly folded (122) one, the fallback (123)
N_WINDOWS, N_READS, FLANK = 6, 40, 64
KEYS = ("DD_NO_FOLD", "DD_FORCE_GBT", "DD_DYNAMIC")


def kind_of(hs, K=2):
    """What the FOLD build does with RO for a haplotype of hs bases (hmm_kernel.hip: foldRO / mirRO), from the length alone."""
    num_s, ro, npos = hs + 2, hs + 1, 64 * K
    if ro % K == K - 1:
        return "folded" if num_s <= npos - 3 else "fallback"
    return "mirrored" if num_s <= npos - 4 else "fallback"


def _rnd(rng, n):
    return "".join(rng.choice(list("ACGT"), n))


def _haps(rng, tail):
    """Eight haplotypes of LENGTHS: one 123-bp sequence with 0..6 bases taken out of its middle (the right end, where RO sits, is shared)."""
    base = _rnd(rng, 123 - len(tail)) + tail
    haps = []
    for i, n in enumerate(LENGTHS):
        cut = 40 + 3 * i
        h = base[:cut] + base[cut + 123 - n:]
        if i == len(LENGTHS) - 1:
            h = h[:20] + ("A" if h[20] != "A" else "C") + h[21:]          # the second 121-bp haplotype differs by a base
        assert len(h) == n
        haps.append(h)
    return haps


def _reads(rng, haps, hap_start, L):
    reads = []

    def cut(h, s, n, q, mq):
        g = _rnd(rng, FLANK) + h + _rnd(rng, FLANK)                        # the haplotype inside random flanks: index FLANK + i = base i
        seq = list(g[FLANK + s:FLANK + s + n])
        for i in range(len(seq)):
            if rng.random() < 0.01:
                seq[i] = str(rng.choice(list("ACGT")))
        qual = [q if rng.random() < 0.8 else 0.9 for _ in seq]
        reads.append(ReadRec("".join(seq), qual, mq, hap_start + s))

    for i in range(N_READS):
        h = haps[int(rng.integers(len(haps)))]
        kind = i % 12
        if kind < 4:                                                        # a third: hanging over the right end by 1..40 bases
            over = int(rng.integers(1, 41))
            cut(h, len(h) + over - L, L, 0.999, 0.9999)
        elif kind < 8:                                                      # a third: inside the haplotype (longer reads: centred on it)
            s = int(rng.integers(0, len(h) - L + 1)) if len(h) >= L else -((L - len(h)) // 2)
            cut(h, s, L, 0.999, 0.9999)
        elif kind < 10:                                                     # hanging over the left end
            cut(h, -int(rng.integers(1, 41)), L, 0.99, 0.999)
        elif kind == 10:                                                    # random sequence, every other one of low base quality (the reads
            q = 0.99 if (i // 12) % 2 else 0.33                             # nearest to the -99 bound under which the left->middle pass is redone)
            reads.append(ReadRec(_rnd(rng, L), [q] * L, 0.5, hap_start + int(rng.integers(0, 20))))
        else:                                                               # 12-bp reads, every other one across the right end
            cut(h, len(h) - (6 if (i // 12) % 2 else 30), 12, 0.999, 0.9999)
    return reads


def _windows(L, seed):
    rng = np.random.default_rng(seed)
    ws = []
    for w in range(N_WINDOWS):
        tail = "ACACACACAC" + "A" * 14 if w == 2 else ""                   # one window on a short-repeat + homopolymer tail: exact ties at RO
        haps = _haps(rng, tail)
        start = 1000 + 500 * w
        # one variant per haplotype, so that var_covered / var_fcov are compared as well
        ws.append(Window(start, haps, _reads(rng, haps, start, L), hap_vars=[[(58, 60)] for _ in haps],
                         hap_var_flanks=[[(50, 70, 1 + (i & 1))] for i in range(len(haps))]))
    return ws


_CACHE = {}


def _case(L, mld, tile):
    """(batch, parameters, oracle results) — built once per shape and shared, never modified."""
    key = (L, mld, tile)
    if key not in _CACHE:
        pb = pack(_windows(L, 20250 + L) * tile)
        p = capi.params_cli_defaults()
        p.maxLengthDel = mld
        _CACHE[key] = (pb, p, _oracle.batch(p, pb, nthreads=16))
    return _CACHE[key]


def _bits(a, k):
    a = np.ascontiguousarray(a, dtype=RESULT_DTYPES[k])
    return a.view(np.uint64) if a.dtype == np.float64 else a


def assert_every_field_equal(got, want, pb, what):
    n = result_lengths(pb)
    assert set(got) == set(RESULT_DTYPES) == set(want)
    for k in RESULT_DTYPES:
        assert n[k] > 0, k
        g, w = _bits(got[k][:n[k]], k), _bits(want[k][:n[k]], k)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, (what, k, bad.size, bad[:5], got[k][bad[:5]], want[k][bad[:5]])


@pytest.fixture()
def clean_env():
    saved = {k: os.environ.pop(k, None) for k in KEYS}
    yield
    for k in KEYS:
        os.environ.pop(k, None)
        if saved[k] is not None:
            os.environ[k] = saved[k]


# maxLengthDel 5 -> D build 6, 10 -> D build 11 (whose FOLD build is the LDS one: the plan's own choice there is the scratch build, which has
# none); 100-bp reads for the LDS builds, 130-bp ones for the K = 2 scratch build; the last case tiles the six windows four times under
# the item counter, so that the grid is smaller than a third of the items
CASES = [("d6-lds", 100, 5, 1, {}, "dd_hmm_kernel<2, 6, false, true, 0, 1>"),
         ("d6-scratch", 130, 5, 1, {"DD_FORCE_GBT": "1"}, "dd_hmm_kernel<2, 6, true, true, 0, 1>"),
         ("d11-lds", 100, 10, 1, {"DD_FORCE_GBT": "0"}, "dd_hmm_kernel<2, 11, false, true, 0, 1>"),
         ("d6-lds-later-items", 100, 5, 4, {"DD_DYNAMIC": "1", "DD_FORCE_GBT": "0"}, "dd_hmm_kernel<2, 6, false, true, 0, 1>")]


@pytest.mark.parametrize("name,L,mld,tile,env,kernel", CASES, ids=[c[0] for c in CASES])
def test_mirrored_ro_equals_oracle_and_one_lane_blocks(lib, clean_env, name, L, mld, tile, env, kernel):
    pb, p, want = _case(L, mld, tile)
    kinds = {kind_of(n) for n in LENGTHS}
    assert kinds == {"mirrored", "folded", "fallback"}, kinds             # all three kinds of haplotype are in the batch ...
    lens = np.diff(pb.a["hap_seq_off"])
    assert {kind_of(int(n)) for n in lens} == kinds and lens.size == N_WINDOWS * tile * len(LENGTHS)   # ... as packed
    assert int((want["status"][:pb.n_pairs] != capi.DD_PAIR_OK).sum()) == 0      # no pair is left out of the comparison
    assert int(want["offHapHMQ"][:pb.n_pairs].sum()) > 0 and int((want["hpos"][:pb.hpos_len] == capi.DD_HPOS_RO).sum()) > 0   # MAP paths do sit in RO

    os.environ.update(env)
    folded = run_host_api(lib, p, pb)
    log = capi.launch_log()
    names = {lib.dd_kernel_name().decode()}
    assert log and all(l["fold"] == 1 and l["K"] == 2 for l in log), log   # the default launch is the FOLD build
    assert names == {kernel}, names
    if tile > 1:                                                            # a workgroup takes a second and a third item
        assert all(l["dynamic"] == 1 for l in log) and max(l["n_haps"] * l["split"] / l["grid"] for l in log) > 2.0, log
    os.environ["DD_NO_FOLD"] = "1"
    plain = run_host_api(lib, p, pb)
    assert all(l["fold"] == 0 for l in capi.launch_log()), capi.launch_log()
    del os.environ["DD_NO_FOLD"]

    assert_every_field_equal(folded, want, pb, name + ": FOLD build against the oracle")
    assert_every_field_equal(plain, want, pb, name + ": one-lane blocks against the oracle")
    assert_every_field_equal(folded, plain, pb, name + ": FOLD build against the one-lane blocks")


def test_kinds_by_length():
    """The lengths the kernel's conditions give at K = 2 (64 K = 128 positions; numS = Hs + 2)."""
    assert [kind_of(n) for n in (117, 118, 119, 120, 121, 122, 123, 124, 125)] == \
        ["mirrored", "folded", "mirrored", "folded", "mirrored", "folded", "fallback", "fallback", "fallback"]
