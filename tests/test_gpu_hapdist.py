"""dd_hapdist_kernel against blockTableHost (host/haplotypes.cpp), word for word: statuses, tables, and everything neither may touch.
blockTableHost itself is compared with the sequential restatement in tests/test_haplotypes_cpu.py."""
import ctypes as C
import random

import numpy as np
import pytest

from dindel_tgi_amd import capi, hapdist, hostlib
from tests import _haplotypes_cases as cases

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A
G = cases.G


def host_twin(a, t):
    """blockTableHost into copies of the (preset) tables."""
    lib = hostlib.load()
    lib.ddh_hap_block_table_flat.argtypes = [C.POINTER(capi.dd_hap_batch), C.POINTER(capi.dd_hap_blocks)]
    lib.ddh_hap_block_table_flat.restype = None
    th = {k: v.copy() for k, v in t.items()}
    b, s = hapdist.host_batch(a), hapdist.host_tables(th)
    lib.ddh_hap_block_table_flat(C.byref(b), C.byref(s))
    return th


def run_both(case_list, slack=8):
    windows, reads = [(c[1], c[2]) for c in case_list], [c[3] for c in case_list]
    a = hapdist.pack(windows, reads)
    preset = hapdist.alloc_tables(len(windows), hapdist.offsets(a), fill=SENTINEL, slack=slack)
    want = host_twin(a, preset)
    _, got = hapdist.block_table(windows, reads, tables={k: v.copy() for k, v in preset.items()})
    log = hapdist.last_launch()
    assert log["guard_trips"] == 0 and log["windows"] == len(windows), log
    return a, got, want, log


def assert_same(got, want):
    for k in want:
        assert np.array_equal(got[k], want[k]), (k, np.flatnonzero(got[k] != want[k])[:8])


def rd(pos, text, rng=None, err=0.0, ins=None, flag=0, letters=None):
    ops = cases.cigar(text)
    return (pos, flag, ops, letters if letters is not None else cases.read_from(G, pos, ops, rng or random.Random(pos), err, ins))


def distinct_block_window(n_other, rs=2000):
    """A window whose block [rs + 4, rs + 8) sees the reference's four bases and n_other other strings, all different."""
    ref = G[rs:rs + 16]
    others = []
    for x in range(256):
        s = bytes(b"ACGT"[(x >> s_) & 3] for s_ in (6, 4, 2, 0))
        if s != ref[4:8] and len(others) < n_other:
            others.append(s)
    return ("distinct%d" % n_other, rs, ref, [(rs + 4, 0, [(0, 4)], s) for s in others])


def edge_cases():
    rng = random.Random(5)
    big = [rd(1190 + rng.randrange(0, 160), "%dM" % rng.randrange(60, 101), rng, err=0.002) for _ in range(700)]
    return [
        ("w256_plain", 1200, G[1200:1456], [rd(1180, "100M", err=0.05), rd(1400, "56M")]),                                  # exactly 64 blocks
        ("w256", 1200, G[1200:1456], [rd(1180, "100M", err=0.02), rd(1300, "40M2I58M", ins=b"AC"), rd(1400, "80M")]),     # 64 x 4: one pass of lanes
        ("w257", 1200, G[1200:1457], [rd(1180, "100M", err=0.02), rd(1380, "90M")]),                                       # the second pass begins
        # cuts off the grid left of position 252 shift the block numbers: a block of the 63rd lane that is covered by some reads only
        ("straddle", 1200, G[1200:1500], [rd(1201, "10M"), rd(1440, "30M", err=0.2), rd(1449, "9M"), rd(1451, "20M", err=0.2), rd(1445, "12M3S")]),
        distinct_block_window(capi.DD_HAPDIST_MAX_DISTINCT - 1),         # exactly the cap with the reference's string
        distinct_block_window(capi.DD_HAPDIST_MAX_DISTINCT),             # one more
        ("good_a", 1000, G[1000:1040], [rd(990, "40M"), rd(1010, "10M1D20M")]),
        ("too_wide", 1000, G[1000:1000 + capi.DD_HAPDIST_MAX_WINDOW + 1], [rd(1100, "50M")]),
        ("good_b", 1000, G[1000:1040], [rd(995, "40M")]),
        ("host", 1000, G[1000:1040], [rd(1001, "10M"), rd(1003, "4M2P4M")]),
        ("good_c", 1000, G[1000:1040], [rd(1002, "30M4S")]),
        ("widest", 1000, G[1000:1000 + capi.DD_HAPDIST_MAX_WINDOW], [rd(900, "100M50D200M"), rd(1990, "60M")]),
        ("reads0", 3000, G[3000:3100], []),
        ("reads1", 3000, G[3000:3100], [rd(3010, "50M")]),
        ("reads700", 1200, G[1200:1360], big),
    ]


@pytest.fixture(scope="module")
def launch_all():
    """The generated and hand-derived windows of the CPU test and the edge cases, in one launch."""
    cs = cases.hand() + cases.generated(300, 1) + cases.generated(20, 2, wide=True) + edge_cases()
    return cs, run_both(cs)


def test_kernel_equals_block_table_host_on_every_window(launch_all):
    cs, (a, got, want, log) = launch_all
    assert_same(got, want)
    st = got["status"][:len(cs)]
    assert (st == capi.DD_HAPDIST_OK).sum() > 300 and (st == capi.DD_HAPDIST_HOST).sum() >= 3


def test_statuses_of_the_edge_cases_and_what_stays_untouched(launch_all):
    cs, (a, got, want, log) = launch_all
    idx = {c[0]: i for i, c in enumerate(cs)}
    st = got["status"]
    for name in ("w256_plain", "w256", "w257", "straddle", "distinct15", "good_a", "good_b", "good_c", "widest", "reads0", "reads1", "reads700"):
        assert st[idx[name]] == capi.DD_HAPDIST_OK, name
    assert st[idx["distinct16"]] == capi.DD_HAPDIST_OVERFLOW and st[idx["too_wide"]] == capi.DD_HAPDIST_TOO_WIDE and st[idx["host"]] == capi.DD_HAPDIST_HOST
    assert got["n_blocks"][idx["w256_plain"]] == 64 and got["n_blocks"][idx["w256"]] > 64 and got["n_blocks"][idx["w257"]] > 64 and got["n_blocks"][idx["reads0"]] == 25
    d = hapdist.decode(a, got, idx["distinct15"])
    assert max(len(b[2]) for b in d["blocks"]) == capi.DD_HAPDIST_MAX_DISTINCT
    for name in ("distinct16", "too_wide", "host"):          # nothing but the status
        w = idx[name]
        for k in ("n_blocks", "n_entries", "n_ins_ops", "n_ins_pos", "left"):
            assert got[k][w] == SENTINEL, (name, k)
        assert (got["blocks"][got["blk_off"][w]:got["blk_off"][w + 1]] == SENTINEL).all()
        assert (got["entries"][2 * got["ent_off"][w]:2 * got["ent_off"][w + 1]] == SENTINEL).all()
    n = len(cs)
    assert (got["blocks"][got["blk_off"][n]:] == SENTINEL).all() and (got["entries"][2 * got["ent_off"][n]:] == SENTINEL).all()
    assert (got["ins_ops"][2 * got["ins_off"][n]:] == SENTINEL).all() and (got["ins_pos"][2 * got["ins_off"][n]:] == SENTINEL).all()
    for w in range(n):                                         # behind each window's own records as well
        if st[w] == capi.DD_HAPDIST_OK:
            assert (got["blocks"][got["blk_off"][w] + got["n_blocks"][w]:got["blk_off"][w + 1]] == SENTINEL).all()
            assert (got["entries"][2 * (got["ent_off"][w] + got["n_entries"][w]):2 * got["ent_off"][w + 1]] == SENTINEL).all()


def test_no_windows():
    a, t = hapdist.block_table([], [])
    assert len(a["win_rs"]) == 0


def test_many_small_windows_so_that_every_wavefront_draws_often():
    rng = random.Random(11)
    cs = []
    for w in range(5000):
        rs = 500 + 4 * (w % 997) + (w % 3)
        cs.append(("s%d" % w, rs, G[rs:rs + 40], [rd(rs - 5 + rng.randrange(0, 20), "%dM" % rng.randrange(10, 40), rng, err=0.05),
                                                  rd(rs + rng.randrange(0, 20), "8M1I9M", rng), rd(rs + 2, "10M2D8M", rng)]))
    a, got, want, log = run_both(cs)
    assert_same(got, want)
    assert (got["status"][:5000] == capi.DD_HAPDIST_OK).all()
    assert log["max_draws"] >= 2 and 2 * log["grid"] * 4 < 5000, log     # at least two windows per wavefront on average


def test_device_entry_on_a_stream_of_its_own(launch_all):
    import torch
    cs, (a, got, want, log) = launch_all
    sub = cs[:40] + cs[-14:]
    dev = hapdist.DeviceBlocks([(c[1], c[2]) for c in sub], [c[3] for c in sub], fill=SENTINEL, slack=16)
    st = torch.cuda.Stream()
    dev.launch(stream=st)
    log2 = hapdist.last_launch()                               # synchronises the stream
    a2, t2 = dev.results()
    assert log2["guard_trips"] == 0 and log2["windows"] == len(sub)
    th = host_twin(a2, hapdist.alloc_tables(len(sub), hapdist.offsets(a2), fill=SENTINEL, slack=16))
    assert_same(t2, th)                                        # the 16 records of sentinels behind each table included
    assert (t2["blocks"][-16:] == SENTINEL).all() and (t2["entries"][-32:] == SENTINEL).all() and (t2["ins_pos"][-32:] == SENTINEL).all()
    dev.launch()                                               # the workspace and the tables serve a second launch
    assert_same(dev.results()[1], th)
    assert hapdist.last_launch()["guard_trips"] == 0
