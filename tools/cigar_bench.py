#!/usr/bin/env python3
"""Time of the device-side getCIGAR launch (dd_cigars_device on a resident batch) next to the likelihood launch it follows, and the bytes
each would send back per pair.
  python tools/cigar_bench.py [--reps 3] [--windows 256] [--ops-cap 8] [--out FILE.json]
Shapes: the headline shape (8 haplotypes x 200 reads x 100 bp, 120-bp haplotypes) and a ragged sample.  Both launches are timed between two
events, best of --reps, after a warm-up of each.  hap_ref_pos is what candidate-haplotype construction gives: the identity for a window's
reference haplotype, one insertion or deletion against it for the others."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from dindel_tgi_amd import capi, synth
from dindel_tgi_amd.device import DeviceBatch


def hap_ref_pos(pb):
    """refHpos of synth.generate's haplotypes from their one variant (hap_var_flank: left flank, right flank, 1 = DEL / 2 = INS)."""
    a = pb.a
    hso, hvo, fl = a["hap_seq_off"], a["hap_var_off"], pb.hap_var_flank.reshape(-1, 3)
    out = np.zeros(int(hso[-1]), np.int32)
    for w in range(pb.n_windows):
        h0, h1 = int(a["win_hap_off"][w]), int(a["win_hap_off"][w + 1])
        ref_len = int(hso[h0 + 1] - hso[h0])
        for g in range(h0, h1):
            n = int(hso[g + 1] - hso[g])
            m = np.arange(n)
            if hvo[g + 1] > hvo[g]:
                left, right, kind = fl[hvo[g]]
                m = np.where(m >= right, m + (ref_len - n), m) if kind == 1 else np.where(m >= right, m - (n - ref_len), np.where(m > left, -1, m))
            out[hso[g]:hso[g + 1]] = m
    return out


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
    ap.add_argument("--windows", type=int, default=256)
    ap.add_argument("--ops-cap", type=int, default=capi.DD_CIGAR_DEFAULT_OPS_CAP)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows = []
    for name, pb in (("headline", synth.generate(args.windows, H=8, R=200, L=100, hap_len=120, seed=7)),
                     ("ragged", synth.generate_ragged(args.windows, seed=0x5EED4))):
        dev = DeviceBatch(pb, capi.params_cli_defaults(), "cuda:0", cigars=True, ops_cap=args.ops_cap, hap_ref_pos=hap_ref_pos(pb))
        st = torch.cuda.current_stream()
        dev.launch(); dev.launch_cigars()
        torch.cuda.synchronize()
        t_lik, t_cig = timed(dev.launch, st, args.reps), timed(dev.launch_cigars, st, args.reps)
        res = dev.results()
        status = res["cigar_status"]
        row = dict(shape=name, windows=pb.n_windows, pairs=pb.n_pairs, ops_cap=args.ops_cap, likelihood_s=min(t_lik), likelihood_s_all=t_lik,
                   cigar_s=min(t_cig), cigar_s_all=t_cig, cigar_share_of_likelihood=min(t_cig) / min(t_lik), cigar_pairs_per_s=pb.n_pairs / min(t_cig),
                   hpos_bytes_per_pair=2.0 * pb.hpos_len / pb.n_pairs, cigar_bytes_per_pair=4 * args.ops_cap + 12,
                   overflow_share=float((status == capi.DD_CIGAR_OVERFLOW).mean()), max_n_ops=int(res["cigar_n_ops"].max()),
                   status_counts={int(k): int(v) for k, v in zip(*np.unique(status, return_counts=True))})
        rows.append(row)
        print(json.dumps(row), flush=True)
        del dev
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
