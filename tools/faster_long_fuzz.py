#!/usr/bin/env python3
"""Randomised GPU-vs-oracle parity campaign of the --faster model's long-window path (DD_OPT_LONG_WINDOWS_FASTER), in the style of
tools/long_window_fuzz.py.
  python tools/faster_long_fuzz.py [--seconds 300] [--seed0 0] [--out profiles/r06/faster_long_fuzz.json]
Every round draws parameters (maxLengthDel 0..31, padCover, maxMismatch; one round in five a set of tests/_param_cases.py on top) and a batch that mixes long windows (haplotypes of 767..4,094 bp
and / or reads of 1,025..4,096 bp; reads from 36 bp) with ordinary ones, runs dd_compute_likelihoods_faster_ex and the oracle's --faster
model (16 threads) and requires every dd_result field bit-equal.  A draw that holds a window beyond the long limits (a variant haplotype
past 4,094 bp) is not run and counted apart.  One line per round; at the first mismatch the seed is printed and the exit code is 1."""
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
from dindel_tgi_amd.batch import alloc_result
from tests import _oracle
from tests.test_gpu_faster import assert_same_faster
from tests.test_gpu_parity import assert_same
from tests._param_cases import PARAM_SETS

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=300)
ap.add_argument("--seed0", type=int, default=0)
ap.add_argument("--out", default="")
args = ap.parse_args()
lib = capi.load()
t0 = time.time()
t_end = t0 + args.seconds
rounds = skipped = pairs = long_pairs = 0
shapes = []
ok = True
while time.time() < t_end:
    seed = args.seed0 + rounds + skipped
    rng = np.random.default_rng(60000 + seed)
    p = capi.params_cli_defaults() if rng.random() < 0.5 else capi.params_struct_defaults()
    p.maxLengthDel = int(rng.integers(0, 32))
    prng = np.random.default_rng(90000 + seed)                          # (a stream of its own: the other draws stay what they were)
    pset = str(prng.choice(list(PARAM_SETS))) if prng.random() < 0.2 else "-"   # one round in five: a set of tests/_param_cases.py on top
    for k, v in PARAM_SETS.get(pset, {}).items():
        setattr(p, k, v)
    p.padCover = int(rng.integers(0, 6))
    p.maxMismatch = int(rng.integers(0, 4))
    kind = int(rng.integers(0, 3))
    if kind == 0:                      # long haplotypes, short reads, many pairs
        hs, L = int(rng.integers(767, 4095)), int(rng.integers(36, 400))
        H, R = int(rng.integers(2, 6)), int(rng.integers(2, 200))
    elif kind == 1:                    # long reads, haplotypes of any length
        hs, L = int(rng.integers(40, 1500)), int(rng.integers(1025, 4097))
        H, R = int(rng.integers(2, 5)), int(rng.integers(2, 24))
    else:                              # the big corner: both long
        hs, L = int(rng.integers(2500, 4095)), int(rng.integers(1025, 4097))
        H, R = int(rng.integers(1, 4)), int(rng.integers(1, 20))
    sub = float(rng.choice([1e-3, 4e-3, 0.02, 0.2]))
    parts = [synth.generate(int(rng.integers(1, 3)), H=H, R=R, L=L, hap_len=hs, seed=seed, max_indel=max(1, min(p.maxLengthDel, 12)), sub_rate=sub,
                            vary_read_len=bool(rng.random() < 0.5) and L <= 1024, mixed_quals=True)]
    if rng.random() < 0.5:             # ordinary windows next to them (same quality tables: mixed_quals)
        parts.append(synth.generate(int(rng.integers(1, 4)), H=int(rng.integers(2, 6)), R=int(rng.integers(5, 30)), L=100, hap_len=150,
                                    seed=seed + 7, mixed_quals=True))
        rng.shuffle(parts)
    pb = synth.concat(parts)
    cls, mx, _ = capi.screen_windows_ex(p, pb, capi.DD_OPT_LONG_WINDOWS_FASTER)
    if (cls == capi.DD_WIN_UNSUPPORTED).any():
        skipped += 1
        continue
    arrs, res = alloc_result(pb, fill=None)
    b = pb.ctypes_batch()
    rc = lib.dd_compute_likelihoods_faster_ex(C.byref(p), C.byref(b), C.byref(res), 0, capi.DD_OPT_LONG_WINDOWS_FASTER)
    want = _oracle.batch(p, pb, nthreads=16, faster=True)
    try:
        assert rc == 0, capi.last_error()
        assert_same_faster(arrs, want, pb)
        if (want["status"][:pb.n_pairs] == 0).all():
            assert_same(arrs, want, pb)
    except AssertionError as e:
        print("MISMATCH seed=%d kind=%d hs=%d L=%d mld=%d: %s" % (seed, kind, hs, L, p.maxLengthDel, str(e)[:300]), flush=True)
        ok = False
        break
    nl = int(sum(pb.win_pair_off[w + 1] - pb.win_pair_off[w] for w in range(pb.n_windows) if cls[w] == capi.DD_WIN_LONG))
    rounds += 1
    pairs += pb.n_pairs
    long_pairs += nl
    shapes.append([kind, hs, L, p.maxLengthDel, nl])
    print("round %d seed %d kind %d hap %d read %d mld %d set %s: %d pairs (%d long) ok" % (rounds, seed, kind, hs, L, p.maxLengthDel, pset, pb.n_pairs, nl), flush=True)
summary = dict(ok=ok, seconds=round(time.time() - t0, 1), rounds=rounds, draws_not_run=skipped, pairs=pairs, long_pairs=long_pairs,
               max_hap=max([s[1] for s in shapes] or [0]), max_read=max([s[2] for s in shapes] or [0]),
               kinds={str(k): sum(1 for s in shapes if s[0] == k) for k in range(3)},
               maxLengthDel_values=sorted({s[3] for s in shapes}))
print(json.dumps(summary))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(summary, f, indent=1)
sys.exit(0 if ok else 1)
