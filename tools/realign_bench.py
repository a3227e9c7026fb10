#!/usr/bin/env python3
"""Time of the realign launch (dd_realign_device: per read the haplotype of the pooled rule and that pair's CIGAR) next to the per-pair CIGAR
launch (dd_cigars_device) on the same resident batch, behind the same likelihood launch, and the bytes each sends back.
  python tools/realign_bench.py [--reps 5] [--windows 256] [--ops-cap 8] [--configs1] [--out FILE.json]
Shapes: the headline shape (8 haplotypes x 200 reads x 100 bp, 120-bp haplotypes; --configs1: 10,000 windows of it) and a ragged sample.
Each launch is timed between two events, --reps times after a warm-up: best, median and the spread (max - min) are reported.  The realign
launch is timed in both modes; DD_REALIGN_PAIR gets a random haplotype pair per window.  hap_ref_pos as in tools/cigar_bench.py."""
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
from tools.cigar_bench import hap_ref_pos, timed


def summary(ts):
    return dict(best_s=min(ts), median_s=float(np.median(ts)), spread_s=max(ts) - min(ts), all_s=ts)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=256)
    ap.add_argument("--configs1", action="store_true", help="the headline shape at 10,000 windows (configs[1])")
    ap.add_argument("--ops-cap", type=int, default=capi.DD_CIGAR_DEFAULT_OPS_CAP)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows = []
    n_head = 10000 if args.configs1 else args.windows
    for name, pb in (("headline", synth.generate(n_head, H=8, R=200, L=100, hap_len=120, seed=7)),
                     ("ragged", synth.generate_ragged(args.windows, seed=0x5EED4))):
        rng = np.random.default_rng(1)
        nh = np.maximum(np.diff(pb.a["win_hap_off"]), 1)
        pairs = np.stack([rng.integers(0, nh), rng.integers(0, nh)], 1).astype(np.int32)
        dev = DeviceBatch(pb, capi.params_cli_defaults(), "cuda:0", cigars=True, realign=True, ops_cap=args.ops_cap, hap_ref_pos=hap_ref_pos(pb),
                          hap_n_indels=(np.diff(pb.a["hap_var_off"]) > 0).astype(np.int32))
        st = torch.cuda.current_stream()
        first_max = lambda: dev.launch_realign(capi.DD_REALIGN_FIRST_MAX)
        pair = lambda: dev.launch_realign(capi.DD_REALIGN_PAIR, win_hap_pair=pairs)
        dev.launch(); dev.launch_cigars(); first_max(); pair()
        torch.cuda.synchronize()
        t_lik = timed(dev.launch, st, min(args.reps, 2))
        t_cig, t_pair, t_first = timed(dev.launch_cigars, st, args.reps), timed(pair, st, args.reps), timed(first_max, st, args.reps)
        res = dev.results()                                      # (of the last launch: the pooled rule)
        on = res["realign_hap"] >= 0
        nr = np.diff(pb.a["win_read_off"])                      # the chosen pair of every read: its rows must be the per-pair launch's
        r_in_win = np.arange(pb.n_reads) - np.repeat(pb.a["win_read_off"][:-1], nr)
        chosen = (np.repeat(pb.win_pair_off[:-1], nr) + res["realign_hap"].astype(np.int64) * np.repeat(nr, nr) + r_in_win)[on]
        same = all(np.array_equal(res["realign_" + k][on], res["cigar_" + k][chosen]) for k in ("status", "n_ops", "ref_off"))
        written = np.arange(args.ops_cap)[None, :] < res["realign_n_ops"][on][:, None]      # (slots beyond a read's count keep what an earlier launch left)
        same = same and np.array_equal(res["realign_ops"][on][written], res["cigar_ops"][chosen][written])
        H_mean = pb.n_pairs / pb.n_reads
        row = dict(shape=name, windows=pb.n_windows, pairs=pb.n_pairs, reads=pb.n_reads, ops_cap=args.ops_cap, likelihood_s=min(t_lik),
                   cigar=summary(t_cig), realign_first_max=summary(t_first), realign_pair=summary(t_pair),
                   realign_over_cigar=min(t_first) / min(t_cig), mean_haplotypes_per_read=H_mean,
                   realign_reads_per_s=pb.n_reads / min(t_first), cigar_pairs_per_s=pb.n_pairs / min(t_cig),
                   realign_bytes_back=pb.n_reads * (4 * args.ops_cap + 16), cigar_bytes_back=pb.n_pairs * (4 * args.ops_cap + 12),
                   hpos_bytes_back=2 * pb.hpos_len, rows_equal_the_per_pair_launch=bool(same), on_hap_share=float(on.mean()),
                   status_counts={int(k): int(v) for k, v in zip(*np.unique(res["realign_status"], return_counts=True))})
        rows.append(row)
        print(json.dumps(row), flush=True)
        del dev
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
