"""The haplotype-to-reference alignment on the device (csrc/hapalign_kernel.hip through dindel_tgi_amd.hapalign).  Everything is exact:
against the output of the reference's own SeqAn library where a fixture exists (tests/golden/hapalign_seqan.json), otherwise against
tests/_hapalign_oracle.py, which tests/test_hapalign_cpu.py pins against the same fixtures."""
import json
import os
import random

import numpy as np
import pytest

from dindel_tgi_amd import capi, hapalign
from tests import _hapalign_oracle as orc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def fixtures():
    return json.load(open(os.path.join(HERE, "golden", "hapalign_seqan.json")))


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def mutated(rng, s, n_sub=2, n_indel=2, max_indel=6):
    s = bytearray(s)
    for _ in range(n_sub):
        s[rng.randrange(len(s))] = rng.choice(b"ACGT")
    for _ in range(n_indel):
        n, p = rng.randint(1, max_indel), rng.randrange(len(s) + 1)
        if rng.random() < 0.5:
            s[p:p] = rand_seq(rng, n)
        elif len(s) > n + 1:
            del s[p:p + n]
    return bytes(s)


def check_against_oracle(refs, haps, pair_ref, got, cache=None):
    """every pair: status 0, score, and the per-base reference offsets (which determine both gapped rows)"""
    off = got["hap_off"]
    cache = {} if cache is None else cache
    assert hapalign.last_launch()["guard_trips"] == 0         # no wavefront iterated more often than the batch has pairs
    for i, h in enumerate(haps):
        key = (refs[pair_ref[i]], h)
        if key not in cache:
            cache[key] = orc.align(*key)
        score, row0, row1, pos = cache[key]
        assert got["status"][i] == capi.DD_ALIGN_OK, i
        assert got["score"][i] == score, (i, got["score"][i], score)
        mine = got["ref_pos"][off[i]:off[i + 1]]
        assert np.array_equal(mine, pos), (i, key, mine.tolist(), pos.tolist())
        if len(h) <= 300:
            assert hapalign.gapped_rows(key[0], h, mine) == (row0, row1), i


def test_all_seqan_fixtures_in_one_launch():
    fx = fixtures()
    refs = [c["ref"].encode("latin-1") for c in fx]
    haps = [c["hap"].encode("latin-1") for c in fx]
    got = hapalign.align_haplotypes(refs, haps, list(range(len(fx))))
    off = got["hap_off"]
    assert np.all(got["status"] == 0)
    for i, c in enumerate(fx):
        assert got["score"][i] == c["score"], (i, c)
        assert hapalign.gapped_rows(refs[i], haps[i], got["ref_pos"][off[i]:off[i + 1]]) == (c["row0"], c["row1"]), (i, c)


def test_lane_and_k_boundaries():
    """haplotype lengths around the multiples of 64 (the rows a lane owns change there) against three reference lengths"""
    rng = random.Random(5)
    refs = [rand_seq(rng, n) for n in (1, 64, 130)]
    haps, pair_ref = [], []
    for n in (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193):
        for r, ref in enumerate(refs):
            # related to the reference where both are long enough, so that the alignment is not one run of mismatches
            src = (ref * (n // len(ref) + 1))[:n]
            haps.append(mutated(rng, src) if n > 8 else rand_seq(rng, n))
            pair_ref.append(r)
    check_against_oracle(refs, haps, pair_ref, hapalign.align_haplotypes(refs, haps, pair_ref))


def test_long_pairs():
    """1,025 x 1,000 (K = 17) and the limit, 4,094 x 4,094 (K = 64, the grid shrunk by the workspace budget)"""
    rng = random.Random(6)
    r1 = rand_seq(rng, 1000)
    h1 = mutated(rng, r1 + rand_seq(rng, 40), 5, 4, 12)[:1025].ljust(1025, b"A")
    r2 = rand_seq(rng, capi.DD_LONG_MAX_HAP_LEN)
    h2 = mutated(rng, r2, 12, 8, 12)[:capi.DD_LONG_MAX_HAP_LEN].ljust(capi.DD_LONG_MAX_HAP_LEN, b"C")
    assert (len(h1), len(h2)) == (1025, 4094)
    refs, haps = [r1, r2], [h1, h2]
    got = hapalign.align_haplotypes(refs, haps, [0, 1])
    log = hapalign.last_launch()
    assert log["grid"] >= 1 and log["ws_bytes"] <= capi.DD_ALIGN_WS_BUDGET + 256 + 4 * log["tile_bytes"]
    check_against_oracle(refs, haps, [0, 1], got)


def test_ties_in_repeats_and_homopolymers():
    """where the indel lands in a repeat is decided by the strict comparisons and the traceback's state machine"""
    refs, haps = [], []
    for unit in (b"A", b"C", b"AC", b"GT", b"ACG", b"TTG"):
        for reps in (3, 7, 30):
            for periods in (1, 2):
                for lf, rf in ((b"", b""), (b"GGTCA", b"CTGAT"), (b"T", b""), (b"", b"C")):
                    long_, short = lf + unit * (reps + periods) + rf, lf + unit * reps + rf
                    refs += [long_, short]
                    haps += [short, long_]
    for a, b in ((8, 10), (10, 8), (1, 70), (70, 1), (64, 65), (65, 64), (100, 130), (130, 100)):
        refs.append(b"A" * a)
        haps.append(b"A" * b)
    pair_ref = list(range(len(refs)))
    check_against_oracle(refs, haps, pair_ref, hapalign.align_haplotypes(refs, haps, pair_ref))


def test_other_bytes():
    rng = random.Random(8)
    base = rand_seq(rng, 40)
    odd = [b"N", b"n", b"a", b"c", b"g", b"t", b"U", b"u", b"\x00", b"\xff", b"R", b"-", b" "]
    refs, haps = [], []
    for k, o in enumerate(odd):
        p = 3 + 2 * k
        spoiled = base[:p] + o + base[p + 1:]
        refs += [spoiled, base, spoiled.lower()]
        haps += [base, spoiled, spoiled]
    refs.append(bytes(range(256)))
    haps.append(bytes(reversed(range(256))))
    pair_ref = list(range(len(refs)))
    check_against_oracle(refs, haps, pair_ref, hapalign.align_haplotypes(refs, haps, pair_ref))


def test_more_pairs_than_wavefronts():
    """20,000 pairs of about 20 x 20 sharing 2,500 references: the persistent grid draws several pairs per wavefront"""
    rng = random.Random(9)
    distinct = [rand_seq(rng, rng.randint(17, 23)) for _ in range(250)]       # 2,500 reference slots, 250 distinct sequences: the checker's work
    refs = [distinct[i % 250] for i in range(2500)]
    per_seq = {r: [mutated(rng, r, 1, 1, 3) for _ in range(3)] + [r] for r in distinct}
    variants = [per_seq[r] for r in refs]
    pair_ref = [i % 2500 for i in range(20000)]
    haps = [variants[r][(i // 2500) % 4] for i, r in enumerate(pair_ref)]
    got = hapalign.align_haplotypes(refs, haps, pair_ref)
    log = hapalign.last_launch()
    assert log["pairs"] == 20000 and log["pairs"] / log["waves"] >= 2 and 2 <= log["max_draws"] <= 20000 and log["guard_trips"] == 0, log
    check_against_oracle(refs, haps, pair_ref, got)


def test_mixed_lengths_in_one_workgroup():
    """a 3-bp pair next to a 700-bp pair: the device entry with a workspace for one workgroup, so that the four wavefronts of that
    workgroup take all six pairs"""
    rng = random.Random(10)
    big = rand_seq(rng, 700)
    refs = [b"ACG", big, b"ACGT", big[:650]]
    haps = [b"AG", mutated(rng, big, 4, 4, 9), b"ACGGT", mutated(rng, big, 3, 3, 9), b"ACG", b"T"]
    pair_ref = [0, 1, 2, 3, 0, 2]
    dev = hapalign.DeviceAlign(refs, haps, pair_ref, "cuda:0", max_workgroups=1)
    dev.launch()
    got = dev.results()
    log = hapalign.last_launch()
    assert log["grid"] == 1 and log["waves"] == 4 and log["max_draws"] >= 2, log
    check_against_oracle(refs, haps, pair_ref, got)
    check_against_oracle(refs, haps, pair_ref, hapalign.align_haplotypes(refs, haps, pair_ref))


def test_statuses_leave_neighbours_alone():
    rng = random.Random(11)
    good = rand_seq(rng, 50)
    too_long = rand_seq(rng, capi.DD_LONG_MAX_HAP_LEN + 1)
    refs = [good, b"", too_long]
    haps = [mutated(rng, good), b"", mutated(rng, good), good, too_long[:300], too_long, good[:30]]
    pair_ref = [0, 0, 0, 1, 2, 0, 0]
    want_status = [0, capi.DD_ALIGN_EMPTY, 0, capi.DD_ALIGN_EMPTY, capi.DD_ALIGN_TOO_LONG, capi.DD_ALIGN_TOO_LONG, 0]
    got = hapalign.align_haplotypes(refs, haps, pair_ref)
    off = got["hap_off"]
    assert got["status"].tolist() == want_status
    for i, st in enumerate(want_status):
        mine = got["ref_pos"][off[i]:off[i + 1]]
        if st:
            assert got["score"][i] == 0 and np.all(mine == -1), i
        else:
            score, _, _, pos = orc.align(refs[pair_ref[i]], haps[i])
            assert got["score"][i] == score and np.array_equal(mine, pos), i


def test_device_entry_on_a_stream_equals_host_entry():
    import torch
    rng = random.Random(12)
    refs = [rand_seq(rng, rng.randint(100, 140)) for _ in range(40)]
    pair_ref = [i % 40 for i in range(400)]
    haps = [mutated(rng, refs[r]) for r in pair_ref]
    want = hapalign.align_haplotypes(refs, haps, pair_ref)
    dev = hapalign.DeviceAlign(refs, haps, pair_ref, "cuda:0")
    stream = torch.cuda.Stream(device="cuda:0")
    for _ in range(2):                                  # the second launch finds the first one's counter in the workspace header
        dev.score.fill_(-7); dev.status.fill_(-7); dev.ref_pos.fill_(-7)
        torch.cuda.synchronize()
        dev.launch(stream)
        got = dev.results()
        for k in ("score", "status", "ref_pos"):
            assert np.array_equal(got[k], want[k]), k
    check_against_oracle(refs, haps, pair_ref, want)
