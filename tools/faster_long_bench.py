#!/usr/bin/env python3
"""Throughput of the --faster model's long-window kernel alone (dd_launch_device_faster_long on a resident batch), and of the 16-thread CPU
oracle's --faster model on windows of the same batch.
  python tools/faster_long_bench.py [--reps 3] [--oracle-threads 16] [--out profiles/r06/faster_long_bench.json]
Shapes: 1,000 / 2,000 / 4,094-bp haplotypes x 150 / 1,500-bp reads (synthetic, Q-mixed).  The model's work per pair is L x <= 16 states, so
the unit is pairs per second and read bases per second.  The GPU number is the launch (prepass + kernel + onHap) between two events, best
of --reps, after a warm-up launch; the main --faster launch of the batch, which only marks these windows, runs before the timed region.
The oracle number is measured on the batch's first windows, one per thread.  The bar: the launch beats the 16-thread oracle."""
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
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--oracle-threads", type=int, default=16)
ap.add_argument("--out", default="")
ap.add_argument("--only", default="", help="HAP,READ: one shape (profiling runs)")
ap.add_argument("--no-oracle", action="store_true")
args = ap.parse_args()
only = tuple(int(v) for v in args.only.split(",")) if args.only else None
lib = capi.load()
rows = []
for hs in (1000, 2000, 4094):
    for L in (150, 1500):
        if only and (hs, L) != only:
            continue
        p = capi.params_cli_defaults()
        H, NW = 4, 32
        R = 256 if L <= 150 else 64                   # 32,768 / 8,192 pairs: several items per workgroup of the persistent grid
        pb = synth.generate(NW, H=H, R=R, L=L, hap_len=hs - 3, seed=hs + L, max_indel=3, sub_rate=1e-3, mixed_quals=True)
        dev = DeviceBatch(pb, p, "cuda:0", long_windows_faster=True)
        assert dev.n_long == pb.n_windows
        st = torch.cuda.current_stream()
        dev.launch_faster()                           # main launch (marks) + long launch: warm-up
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            rc = lib.dd_launch_device_faster_long(C.byref(p), C.byref(dev.db), C.byref(dev.dr), C.c_void_p(dev.long_ws.data_ptr()),
                                                  dev.long_ws_bytes, C.c_void_p(st.cuda_stream))
            assert rc == 0, capi.last_error()
            e1.record(st)
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / 1e3)
        log = capi.faster_long_launch_log()[0]
        t = min(times)
        nw = min(pb.n_windows, args.oracle_threads)
        sub_pairs = pb.n_pairs * nw // pb.n_windows
        t0 = time.time()
        if not args.no_oracle:
            _oracle.batch(p, pb, nthreads=args.oracle_threads, first_window=0, n_win=nw, faster=True)
        to = max(time.time() - t0, 1e-9)
        gpu, cpu = pb.n_pairs / t, (sub_pairs / to if not args.no_oracle else float("nan"))
        row = dict(hap=hs, read=L, pairs=pb.n_pairs, gpu_s=round(t, 6), gpu_s_all=[round(x, 6) for x in times], gpu_pairs_per_s=gpu,
                   gpu_read_bases_per_s=gpu * L, oracle_threads=args.oracle_threads, oracle_pairs=sub_pairs, oracle_s=round(to, 4),
                   oracle_pairs_per_s=cpu, speedup=gpu / cpu, grid=log["grid"], max_pairs_per_wg=log["max_pairs_per_wg"],
                   max_items_per_wg=log["max_items_per_wg"], ws_mib=round(log["ws_bytes"] / 2**20, 1), lds_block=log["lds_block"])
        rows.append(row)
        print(json.dumps(row), flush=True)
        del dev
        torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
