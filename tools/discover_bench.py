#!/usr/bin/env python3
"""The one command against its parts: wall time of `dindel_gpu --discover` next to the tools run one after the other.
  python tools/discover_bench.py [--windows 2000] [--reps 3] [--parent-host DIR] [--dir /tmp/discover_bench] [--out FILE.json]
The sample is that of tools/hapstage_bench.py part (3): tools/n2_pipeline_bench.py's generator, whose reads carry their window's indel in
their CIGARs.  Timed, best of --reps after a warm-up run each:
  one     dindel_gpu --discover --bamFile ... --ref ...            (its "discovery_seconds:" line gives the stage's share)
  parts   dindel_candidates --analysis getCIGARindels, dindel_windows --oneFile on its output, and dindel_gpu --ref --varFile on the window
          file made once — dindel_candidates and dindel_gpu taken from --parent-host (a build of the parent commit; default: this tree's)
The stage is a barrier in front of the loop and the same code runs either way, so the one command is not expected to be faster; what it
saves is one process start-up with its HIP context.  Reported: the walls, their spreads (max - min of the runs), the difference
one - sum(parts) and whether it stays within the summed spread of the three runs."""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from hapstage_bench import HOST, best, env, run_timed, spread

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-host", default="")
    ap.add_argument("--dir", default="/tmp/discover_bench")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    d = args.dir
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "n2_pipeline_bench.py"), "--windows", str(args.windows), "--dir", d, "--reps", "1", "--procs", "16"],
                       capture_output=True, text=True)
    assert "generated %d windows" % args.windows in r.stdout, r.stdout + r.stderr
    parent = args.parent_host or HOST
    bam, ref = d + "/reads.bam", d + "/ref.fa"
    one, chain = d + "/one", d + "/chain"

    t_one = run_timed([os.path.join(HOST, "dindel_gpu"), "--discover", "--bamFile", bam, "--ref", ref, "--outputFile", one, "--quiet", "--timing"], args.reps)
    stage = [float(re.search(r"^discovery_seconds: ([0-9.e+-]+)", x[2], re.M).group(1)) for x in t_one]
    t_cand = run_timed([os.path.join(parent, "dindel_candidates"), "--analysis", "getCIGARindels", "--bamFile", bam, "--ref", ref, "--outputFile", chain, "--quiet"], args.reps)
    t_win = run_timed([os.path.join(HOST, "dindel_windows"), "-i", chain + ".variants.txt", "--oneFile", chain + ".windows.txt", "--quiet"], args.reps)
    t_loop = run_timed([os.path.join(parent, "dindel_gpu"), "--bamFile", bam, "--varFile", chain + ".windows.txt", "--ref", ref, "--outputFile", chain, "--quiet", "--timing"],
                       args.reps)
    same = all(open(one + e, "rb").read() == open(chain + e, "rb").read() for e in (".variants.txt", ".libraries.txt", ".windows.txt", ".glf.txt"))
    parts = {"dindel_candidates": t_cand, "dindel_windows": t_win, "dindel_gpu": t_loop}
    sum_parts = sum(best(t) for t in parts.values())
    spread_parts = sum(spread(t) for t in parts.values())
    row = dict(windows_in_sample=args.windows, window_lines=open(one + ".windows.txt").read().count("\n"), reps=args.reps, parent_host=parent, outputs_equal=same,
               one_wall_s=best(t_one), one_wall_all=[x[0] for x in t_one], one_spread_s=spread(t_one),
               stage_s=min(stage), stage_all=stage, stage_share_of_one=min(stage) / best(t_one),
               parts={k: dict(wall_s=best(t), wall_all=[x[0] for x in t], spread_s=spread(t)) for k, t in parts.items()},
               sum_of_parts_s=sum_parts, spread_of_parts_s=spread_parts, one_minus_parts_s=best(t_one) - sum_parts,
               within_spread=best(t_one) - sum_parts <= max(spread_parts, spread(t_one)))
    print(json.dumps(row))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(row, open(args.out, "w"), indent=1, sort_keys=True)
        open(args.out, "a").write("\n")
