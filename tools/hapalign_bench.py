#!/usr/bin/env python3
"""Time of the haplotype alignment launch (dd_align_haplotypes_device on a resident batch) next to the likelihood launch of the same
number of windows in the headline shape (BASELINE.json configs[1]: 8 haplotypes x 200 reads x 100 bp, 120-bp haplotypes), on the same
card in the same job.
  python tools/hapalign_bench.py [--reps 3] [--windows 10000] [--out FILE.json]
The alignment batch: --windows windows x 8 haplotypes of 118 ... 132 bp (the reference with up to two substitutions and up to two
indels) against references of 121 ... 125 bp, which is what DetInDel::alignHaplotypes (DInDel.cpp:1427-1524) sees per window.  Both
launches are timed between two events, best of --reps, after a warm-up of each.  Prints DP cells per second of the alignment launch and
its time as a share of the likelihood launch."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from dindel_tgi_amd import capi, hapalign, synth
from dindel_tgi_amd.device import DeviceBatch


def make_batch(windows, haps_per_window=8, seed=0xA11C):
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    refs, haps, pair_ref = [], [], []
    for w in range(windows):
        ref = letters[rng.integers(0, 4, int(rng.integers(121, 126)))]
        refs.append(ref.tobytes())
        for _ in range(haps_per_window):
            h = ref.copy()
            for _ in range(int(rng.integers(0, 3))):
                h[int(rng.integers(0, len(h)))] = letters[int(rng.integers(0, 4))]
            for _ in range(int(rng.integers(0, 3))):
                n, p = int(rng.integers(1, 5)), int(rng.integers(1, len(h) - 5))
                h = np.concatenate([h[:p], letters[rng.integers(0, 4, n)], h[p:]]) if rng.random() < 0.5 else np.concatenate([h[:p], h[p + n:]])
            h = h[:132]
            if len(h) < 118:
                h = np.concatenate([h, letters[rng.integers(0, 4, 118 - len(h))]])
            haps.append(h.tobytes())
            pair_ref.append(w)
    return refs, haps, pair_ref


def timed(fn, st, reps):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st); fn(); e1.record(st)
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 1e3)
    return ts


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=10000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    refs, haps, pair_ref = make_batch(args.windows)
    cells = int(sum(len(refs[r]) * len(h) for r, h in zip(pair_ref, haps)))
    st = torch.cuda.current_stream()
    al = hapalign.DeviceAlign(refs, haps, pair_ref, "cuda:0")
    al.launch(st)
    got = al.results()
    assert np.all(got["status"] == capi.DD_ALIGN_OK)
    t_al = timed(lambda: al.launch(st), st, args.reps)
    log = hapalign.last_launch()
    pb = synth.generate(args.windows, H=8, R=200, L=100, hap_len=120, seed=0x9E3779B9)
    dev = DeviceBatch(pb, capi.params_cli_defaults(), "cuda:0")
    dev.launch()
    torch.cuda.synchronize()
    t_lik = timed(dev.launch, st, args.reps)
    row = dict(windows=args.windows, pairs=len(haps), hap_len=[min(map(len, haps)), max(map(len, haps))], ref_len=[min(map(len, refs)), max(map(len, refs))],
               cells=cells, align_s=min(t_al), align_s_all=t_al, align_cells_per_s=cells / min(t_al), align_ms_per_window=1e3 * min(t_al) / args.windows,
               likelihood_s=min(t_lik), likelihood_s_all=t_lik, align_share_of_likelihood=min(t_al) / min(t_lik), launch=log,
               score_sum=int(got["score"].astype(np.int64).sum()))
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(row, f, indent=1)
