#!/usr/bin/env python3
"""Randomised GPU-vs-oracle parity campaign of the long-window path (DD_OPT_LONG_WINDOWS), in the style of tests/fuzz_campaign.py.
  python tools/long_window_fuzz.py [--seconds 600] [--seed0 0] [--out profiles/r05/long_window_fuzz.json]
Every round draws parameters (maxLengthDel 0..31, padCover, maxMismatch; one round in five a set of tests/_param_cases.py on top, bMid; in a quarter of the rounds mapUnmappedReads with mate
arrays and two insert-size libraries) and a batch that mixes long windows (haplotypes of 575..4,094 bp, reads of 36..4,096 bp) with ordinary
ones, runs dd_compute_likelihoods_ex and the oracle (16 threads) and requires every dd_result field bit-equal.  A draw that holds a window
the long path does not take either (a variant haplotype past 4,094 bp) is not run and counted apart.  One line per round; at the first
mismatch the seed is printed and the exit code is 1."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from dindel_tgi_amd import capi, synth
from dindel_tgi_amd.batch import PackedBatch, alloc_result
from tests import _oracle
from tests.test_gpu_parity import assert_same
from tests._param_cases import PARAM_SETS

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=600)
ap.add_argument("--seed0", type=int, default=0)
ap.add_argument("--out", default="")
args = ap.parse_args()
lib = capi.load()
t0 = time.time()
t_end = t0 + args.seconds
rounds = skipped = mate_rounds = pairs = long_pairs = cells = 0
shapes = []
ok = True
while time.time() < t_end:
    seed = args.seed0 + rounds + skipped
    rng = np.random.default_rng(90000 + seed)
    p = capi.params_cli_defaults() if rng.random() < 0.5 else capi.params_struct_defaults()
    p.maxLengthDel = int(rng.integers(0, 32))
    prng = np.random.default_rng(90000 + seed)                          # (a stream of its own: the other draws stay what they were)
    pset = str(prng.choice(list(PARAM_SETS))) if prng.random() < 0.2 else "-"   # one round in five: a set of tests/_param_cases.py on top
    for k, v in PARAM_SETS.get(pset, {}).items():
        setattr(p, k, v)
    p.padCover = int(rng.integers(0, 6))
    p.maxMismatch = int(rng.integers(0, 4))
    p.bMid = -1 if rng.random() < 0.8 else int(rng.integers(0, 2000))
    kind = int(rng.integers(0, 4))
    if kind == 0:                      # long haplotypes, short reads
        hs, L = int(rng.integers(767, 2600)), int(rng.integers(36, 260))
    elif kind == 1:                    # long reads, haplotypes of any main length
        hs, L = int(rng.integers(max(20, p.maxLengthDel + 4), 766)), int(rng.integers(1025, 2600))
    elif kind == 2:                    # 575..766 bp (long only at maxLengthDel >= 12) with moderate reads
        hs, L = int(rng.integers(575, 767)), int(rng.integers(60, 400))
    else:                              # the big corner: both long, few pairs
        hs, L = int(rng.integers(2500, 4095)), int(rng.integers(1025, 4097))
    H = int(rng.integers(1, 4)) if kind == 3 else int(rng.integers(2, 6))
    R = int(rng.integers(1, 3)) if kind == 3 else int(rng.integers(2, 10))
    # the oracle caps its variant lists at 1,056 entries per pair: few mismatches on long reads
    sub = float(rng.choice([1e-3, 4e-3, 0.02])) if L <= 1000 else 1e-3
    parts = [synth.generate(int(rng.integers(1, 3)), H=H, R=R, L=L, hap_len=hs, seed=seed, max_indel=max(1, p.maxLengthDel), sub_rate=sub,
                            vary_read_len=bool(rng.random() < 0.5) and L <= 1024, mixed_quals=True)]
    if rng.random() < 0.5:             # ordinary windows next to them (same quality tables: mixed_quals)
        parts.append(synth.generate(int(rng.integers(1, 4)), H=int(rng.integers(2, 6)), R=int(rng.integers(5, 30)), L=100, hap_len=150,
                                    seed=seed + 7, mixed_quals=True))
        rng.shuffle(parts)
    pb = synth.concat(parts)
    with_mates = bool(rng.random() < 0.25)
    if with_mates:                     # the insert-size prior at the join: paired reads, mates on either strand, two libraries
        p.mapUnmappedReads = 1
        n = pb.n_reads
        flags = (2 * (rng.random(n) < 0.8) | 4 * (rng.random(n) < 0.1) | 8 * (rng.random(n) < 0.5) | 16 * (rng.random(n) < 0.9)).astype(np.uint8)
        arrays = dict(pb.a)
        arrays["read_flags"] = flags | (pb.a["read_flags"] & 1)
        probs = [rng.random(int(rng.integers(50, 1200))) + 0.05 for _ in range(2)]
        probs = [x / x.sum() for x in probs]
        mate = dict(read_mate_pos=(pb.a["read_start"].astype(np.int64) + rng.integers(-800, 800, n)).astype(np.int32),
                    read_mate_len=np.where(rng.random(n) < 0.1, -1, rng.integers(50, 300, n)).astype(np.int32),
                    read_lib=rng.integers(0, 2, n).astype(np.uint8), lib_off=np.array([0, len(probs[0]), len(probs[0]) + len(probs[1])], np.int32),
                    lib_prob=np.concatenate(probs), lib_p95=np.array([float(x.min()) for x in probs]))
        pb = PackedBatch(hap_var_flank=pb.hap_var_flank, mate=mate, **arrays)
    cls, mx, _ = capi.screen_windows_ex(p, pb)
    if (cls == capi.DD_WIN_UNSUPPORTED).any():
        skipped += 1
        continue
    arrs, res = alloc_result(pb, fill=None)
    b = pb.ctypes_batch()
    rc = lib.dd_compute_likelihoods_ex(C.byref(p), C.byref(b), C.byref(res), 0, capi.DD_OPT_LONG_WINDOWS)
    want = _oracle.batch(p, pb, nthreads=16 if kind != 3 else 4)
    try:
        assert rc == 0, capi.last_error()
        assert_same(arrs, want, pb)
    except AssertionError as e:
        print("MISMATCH seed=%d kind=%d hs=%d L=%d mld=%d: %s" % (seed, kind, hs, L, p.maxLengthDel, str(e)[:300]), flush=True)
        ok = False
        break
    nl = int(sum(pb.win_pair_off[w + 1] - pb.win_pair_off[w] for w in range(pb.n_windows) if cls[w] == capi.DD_WIN_LONG))
    rounds += 1
    mate_rounds += int(with_mates)
    pairs += pb.n_pairs
    long_pairs += nl
    cells += pb.cells
    shapes.append([kind, hs, L, p.maxLengthDel, nl])
    print("round %d seed %d kind %d hap %d read %d mld %d set %s%s: %d pairs (%d long) ok" % (rounds, seed, kind, hs, L, p.maxLengthDel,
          pset, " mates" if with_mates else "", pb.n_pairs, nl), flush=True)
summary = dict(ok=ok, seconds=round(time.time() - t0, 1), rounds=rounds, rounds_with_mates=mate_rounds, draws_not_run=skipped, pairs=pairs, long_pairs=long_pairs, cells=cells,
               max_hap=max([s[1] for s in shapes] or [0]), max_read=max([s[2] for s in shapes] or [0]),
               kinds={str(k): sum(1 for s in shapes if s[0] == k) for k in range(4)},
               maxLengthDel_values=sorted({s[3] for s in shapes}))
print(json.dumps(summary))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(summary, f, indent=1)
sys.exit(0 if ok else 1)
