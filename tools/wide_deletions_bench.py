#!/usr/bin/env python3
"""Throughput of the long-window kernel's wide build (dd_launch_device_wide, maxLengthDel above 31) on a resident batch of the flagship shape
— 120-bp haplotypes, 100-bp reads, 8 haplotypes x 50 reads per window — next to the main kernels' D = 32 build at maxLengthDel 31 on the
same batch and to the 16-thread CPU oracle.
  python tools/wide_deletions_bench.py [--windows 256] [--reps 3] [--oracle-threads 16] [--out profiles/wide/wide_bench.json]
A launch is timed between two events on the stream, after one warm-up launch; pairs/s = pairs of the batch / the best of --reps launches
(every repetition is kept in the record).  The oracle runs --oracle-threads windows, one per thread.  Cost grows with min(D, Hs)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from dindel_tgi_amd import capi, synth
from dindel_tgi_amd.device import DeviceBatch
from tests import _oracle

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=256)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--oracle-threads", type=int, default=16)
ap.add_argument("--out", default="")
args = ap.parse_args()
pb = synth.generate(args.windows, H=8, R=50, L=100, hap_len=120, seed=20261021, mixed_quals=True)
rows = []
for mld in (31, 40, 100):
    p = capi.params_cli_defaults()
    p.maxLengthDel = mld
    wide = mld > capi.DD_MAX_LENGTH_DEL
    dev = DeviceBatch(pb, p, "cuda:0", long_windows=True, wide_deletions=wide)
    assert dev.wide == wide and (not wide or dev.n_long == pb.n_windows)
    st = torch.cuda.current_stream()
    dev.launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        dev.launch()
        e1.record(st)
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3)
    got = dev.results()
    nw = min(pb.n_windows, args.oracle_threads)
    t0 = time.time()
    want = _oracle.batch(p, pb, nthreads=args.oracle_threads, first_window=0, n_win=nw)
    to = max(time.time() - t0, 1e-9)
    n_sub = int(pb.win_pair_off[nw])
    same = all(got[k][:n_sub].tobytes() == want[k][:n_sub].tobytes() for k in ("ll", "status", "offHap", "numIndels"))
    log = capi.long_launch_log() if wide else []
    row = dict(maxLengthDel=mld, build="long kernel, wide" if wide else "main kernels, D = 32", windows=pb.n_windows, pairs=pb.n_pairs,
               gpu_s=[round(t, 6) for t in times], gpu_pairs_per_s=pb.n_pairs / min(times), oracle_threads=args.oracle_threads, oracle_pairs=n_sub,
               oracle_s=round(to, 3), oracle_pairs_per_s=n_sub / to, equal_to_oracle_on_its_pairs=bool(same),
               K=log[0]["K"] if log else None, grid=log[0]["grid"] if log else None, max_pairs_per_wg=log[0]["max_pairs_per_wg"] if log else None)
    rows.append(row)
    print(json.dumps(row), flush=True)
    del dev
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
