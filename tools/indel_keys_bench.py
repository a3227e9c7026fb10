#!/usr/bin/env python3
"""The launch of the --faster model's indel-map key count (dd_indel_keys_device) next to the likelihood launch it follows.
  python tools/indel_keys_bench.py [--windows 10000] [--reps 5] [--host-threads 16] [--out FILE.json]
A resident batch in the flagship shape (BASELINE.json configs[1]: --windows windows x 8 haplotypes x 200 reads of 100 bp, haplotypes of
120 bp; 50 generated windows tiled).  Reported, each the best of --reps after a warm-up with all repetitions beside it: the key launch
between two events behind dd_launch_device_faster, that likelihood launch itself, the bytes the key launch reads (the pairs' hpos) and the
rate that makes, the bytes either way of bringing the indel count back to the host would copy (2 against 2 L per pair), the CPU evaluation
of the first --host-windows windows on --host-threads threads scaled to the batch, and whether device and CPU agree on every pair."""
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


def timed(st, fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st); fn(); e1.record(st)
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--host-windows", type=int, default=500)
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("indel_keys_bench needs a GPU")
    gen = min(a.windows, 50)
    base = synth.generate(gen, H=8, R=200, L=100, hap_len=120, seed=0x9E3779B9)
    reps = -(-a.windows // gen)
    pb = synth.tile(base, reps)
    if pb.n_windows != a.windows:
        pb = pb.slice_windows(0, a.windows)
    dev = DeviceBatch(pb, capi.params_cli_defaults(), "cuda:0", indel_keys=True)
    st = torch.cuda.current_stream(dev.device)
    t_faster = timed(st, dev.launch_faster, a.reps)
    t_keys = timed(st, dev.launch_indel_keys, a.reps)
    res = dev.results()
    keys = res["indel_keys"]
    hw = min(a.host_windows, pb.n_windows)
    sub = pb.slice_windows(0, hw)
    hts = []
    for _ in range(2):
        t0 = time.time()
        want = capi.indel_keys_host(sub, res["hpos"][:sub.hpos_len], res["status"][:sub.n_pairs], nthreads=a.host_threads)
        hts.append(time.time() - t0)
    whole = capi.indel_keys_host(pb, res["hpos"], res["status"], nthreads=a.host_threads)
    hpos_bytes = 2 * int(pb.hpos_len)
    out = {"device": torch.cuda.get_device_name(0), "windows": pb.n_windows, "pairs": int(pb.n_pairs), "read_len": 100,
           "keys_launch_s": min(t_keys), "keys_launch_s_all": t_keys, "faster_launch_s": min(t_faster), "faster_launch_s_all": t_faster,
           "keys_over_faster": min(t_keys) / min(t_faster), "ns_per_pair": min(t_keys) / pb.n_pairs * 1e9,
           "hpos_bytes_read": hpos_bytes, "hpos_read_GB_per_s": hpos_bytes / min(t_keys) / 1e9,
           "bytes_back_with_keys": 2 * int(pb.n_pairs), "bytes_back_with_hpos": hpos_bytes,
           "host_threads": a.host_threads, "host_windows": hw, "host_s_sample": min(hts), "host_s_scaled_to_batch": min(hts) * pb.n_windows / hw,
           "equal_on_every_pair": bool(np.array_equal(whole, keys) and np.array_equal(want, keys[:sub.n_pairs])),
           "pairs_with_keys": int((keys > 0).sum()), "max_keys": int(keys.max()), "overflow_pairs": int((keys == capi.DD_INDEL_KEYS_OVERFLOW).sum())}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
