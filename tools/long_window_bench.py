#!/usr/bin/env python3
"""Throughput of the long-window kernel alone (dd_launch_device_long on a resident batch), and of the 16-thread CPU oracle on the same pairs.
  python tools/long_window_bench.py [--reps 3] [--oracle-threads 16] [--out profiles/r05/long_window_bench.json]
Shapes: 1,000 / 2,000 / 4,094-bp haplotypes x 150 / 1,500-bp reads at maxLengthDel 5 and 20 (synthetic, Q-mixed).  A cell is one
(read base, haplotype base) pair: L x Hs per pair.  The GPU number is the long launch between two events (the main launch of the batch,
which only marks these windows, runs before the timed region); the oracle number is measured on a subset of the pairs."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from dindel_tgi_amd import capi, synth
from dindel_tgi_amd.device import DeviceBatch
from tests import _oracle

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--oracle-threads", type=int, default=16)
ap.add_argument("--out", default="")
ap.add_argument("--only", default="", help="HAP,READ,MLD: one shape (profiling runs)")
ap.add_argument("--no-oracle", action="store_true")
args = ap.parse_args()
only = tuple(int(v) for v in args.only.split(",")) if args.only else None
lib = capi.load()
rows = []
for hs in (1000, 2000, 4094):
    for L in (150, 1500):
        for mld in (5, 20):
            if only and (hs, L, mld) != only:
                continue
            p = capi.params_cli_defaults()
            p.maxLengthDel = mld
            cells_pair = hs * L
            n_pairs = int(max(64, min(4096, 1.2e9 // cells_pair)))
            H, NW = 4, 32
            R = max(1, n_pairs // (H * NW))
            pb = synth.generate(NW, H=H, R=R, L=L, hap_len=hs - 3, seed=hs + L + mld, max_indel=min(3, mld), sub_rate=1e-3, mixed_quals=True)
            dev = DeviceBatch(pb, p, "cuda:0", long_windows=True)
            assert dev.n_long == pb.n_windows
            st = torch.cuda.current_stream()
            dev.launch()                                  # main launch (marks) + long launch: warm-up
            torch.cuda.synchronize()
            times = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                rc = lib.dd_launch_device_long(C.byref(p), C.byref(dev.db), C.byref(dev.dr), C.c_void_p(dev.long_ws.data_ptr()),
                                               dev.long_ws_bytes, C.c_void_p(st.cuda_stream))
                assert rc == 0, capi.last_error()
                e1.record(st)
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1) / 1e3)
            log = capi.long_launch_log()[0]
            t = min(times)
            gpu = pb.cells / t
            # oracle: the first windows, one per thread (the oracle runs a window per thread)
            nw = min(pb.n_windows, args.oracle_threads)
            sub_cells = pb.cells * nw // pb.n_windows
            t0 = time.time()
            if not args.no_oracle:
                _oracle.batch(p, pb, nthreads=args.oracle_threads, first_window=0, n_win=nw)
            to = max(time.time() - t0, 1e-9)
            cpu = sub_cells / to if not args.no_oracle else float("nan")
            row = dict(hap=hs, read=L, maxLengthDel=mld, pairs=pb.n_pairs, cells=int(pb.cells), gpu_s=round(t, 5), gpu_cells_per_s=gpu,
                       oracle_threads=args.oracle_threads, oracle_cells=sub_cells, oracle_s=round(to, 3), oracle_cells_per_s=cpu,
                       speedup=gpu / cpu, K=log["K"], grid=log["grid"], max_pairs_per_wg=log["max_pairs_per_wg"], ws_mib=round(log["ws_bytes"] / 2**20, 1),
                       lds_block=log["lds_block"])
            rows.append(row)
            print(json.dumps(row), flush=True)
            del dev
            torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
