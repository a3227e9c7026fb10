#!/usr/bin/env python3
"""Time of the pair launch (dd_diploid_pairs_device: every window's MAP haplotype pair, chosen and certified) and of the pair + realign chain
(dd_realign_device, DD_REALIGN_PAIR, reading the pairs on the device), next to the per-pair CIGAR launch and the likelihood launch they
follow, on the same resident batch; the bytes each sends back; and how many windows the kernel does not certify, by state.
  python tools/diploid_pair_bench.py [--reps 5] [--windows 256] [--ops-cap 8] [--configs1] [--out FILE.json]
Shapes and method as tools/realign_bench.py (events around each launch on a resident batch, --reps times after a warm-up: best, median,
spread).  The prior is a stand-in for getHaplotypePrior with the same structure: log(1e-4) per haplotype of the pair that carries a variant."""
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
from tools.realign_bench import summary


def stand_in_prior(pb):
    has_var = (np.diff(pb.a["hap_var_off"]) > 0).astype(np.float64) * np.log(1e-4)
    parts = []
    for w in range(pb.n_windows):
        v = has_var[pb.a["win_hap_off"][w]:pb.a["win_hap_off"][w + 1]]
        parts.append((v[:, None] + v[None, :]).reshape(-1))
    return np.concatenate(parts) if parts else np.zeros(0)


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
        prior = stand_in_prior(pb)
        dev = DeviceBatch(pb, capi.params_cli_defaults(), "cuda:0", cigars=True, realign=True, ops_cap=args.ops_cap, hap_ref_pos=hap_ref_pos(pb),
                          hap_n_indels=(np.diff(pb.a["hap_var_off"]) > 0).astype(np.int32), diploid_prior=prior)
        st = torch.cuda.current_stream()

        def chain():
            dip = dev.launch_diploid_pairs()
            dev.launch_realign(capi.DD_REALIGN_PAIR, win_hap_pair=dip["pair"])
        dev.launch(); dev.launch_cigars(); chain()
        torch.cuda.synchronize()
        t_lik = timed(dev.launch, st, min(args.reps, 2))
        t_cig, t_pair, t_chain = timed(dev.launch_cigars, st, args.reps), timed(dev.launch_diploid_pairs, st, args.reps), timed(chain, st, args.reps)
        res, dp = dev.results(), dev.diploid_pair_results()
        twin = capi.diploid_pairs_host(pb.a["win_hap_off"], pb.a["win_read_off"], res["ll"], prior, res["status"], nthreads=8)
        same = all(np.asarray(dp[k]).tobytes() == np.asarray(twin[k]).tobytes() for k in capi.DIPLOID_PAIR_FIELDS)
        states = {int(k): int(v) for k, v in zip(*np.unique(dp["state"], return_counts=True))}
        cert = dp["state"] == capi.DD_DIPPAIR_CERTIFIED
        row = dict(shape=name, windows=pb.n_windows, pairs=pb.n_pairs, reads=pb.n_reads, ops_cap=args.ops_cap, likelihood_s=min(t_lik),
                   cigar=summary(t_cig), pair=summary(t_pair), pair_and_realign=summary(t_chain),
                   chain_over_cigar=min(t_chain) / min(t_cig), pair_windows_per_s=pb.n_windows / min(t_pair),
                   chain_bytes_back=pb.n_reads * (4 * args.ops_cap + 16) + pb.n_windows * 36, cigar_bytes_back=pb.n_pairs * (4 * args.ops_cap + 12),
                   hpos_bytes_back=2 * pb.hpos_len, equals_the_cpu_evaluation=bool(same), state_counts=states,
                   uncertified_share=float(1.0 - cert.mean()) if len(cert) else 0.0,
                   smallest_certified_gap=float(dp["gap"][cert].min()) if cert.any() else None,
                   largest_margin=float(dp["margin"].max()) if len(cert) else None)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del dev
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
