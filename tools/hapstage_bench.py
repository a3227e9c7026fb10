#!/usr/bin/env python3
"""The haplotype stage of dindel_gpu --ref and the variants kernel behind the alignment launch.
  python tools/hapstage_bench.py [--reps 3] [--windows 10000] [--tool-windows 2000] [--loop-windows 2000] [--parent-host DIR] [--out FILE.json]
Reported, best of --reps after a warm-up:
  (1) the variants launch (dd_hap_variants_device) for --windows windows x 8 haplotypes of tools/hapalign_bench.py's shape, between two
      events on a resident batch, next to the alignment launch it follows; bytes back per pair either way (records + summary against
      the slice);
  (2) dindel_hapalign on the W / R / H file dindel_haplotypes writes for a sample of tools/n2_pipeline_bench.py's generator
      (--tool-windows windows), with the variants kernel and with --hostConvert: wall and CPU seconds, a run over the file's first window
      (start-up, device initialisation) taken off both;
  (3) the window loop: dindel_gpu --ref on a sample of the same generator (--loop-windows windows), windows/s and prepare-stage seconds
      per window from its --timing line, with and without --hostConvert and for several --prepareThreads; next to it the chain
      dindel_haplotypes -> dindel_hapalign -> dindel_gpu --hapFile (wall times summed) and dindel_gpu --hapFile alone, run with the tools
      under --parent-host (a build of the parent commit: DIR/dindel_gpu ...; default: this tree's, dindel_hapalign with --hostConvert).
The variants of every alignment restate convertAlignment and getFlankingCoordinatesBetter (ObservationModelSeqAn.hpp:37-269)."""
import argparse
import json
import os
import re
import resource
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
from dindel_tgi_amd import capi, hapalign
from hapalign_bench import make_batch, timed

HOST = os.path.join(ROOT, "dindel_tgi_amd", "host")


def env():
    e = dict(os.environ)
    e["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + e.get("LD_LIBRARY_PATH", "")
    return e


def run_timed(cmd, reps, warm=1):
    """[(wall, cpu, stdout)] of `reps` runs after `warm` warm-up runs"""
    out = []
    for _ in range(reps + warm):
        u0 = resource.getrusage(resource.RUSAGE_CHILDREN)
        t = time.time()
        r = subprocess.run(cmd, env=env(), capture_output=True, text=True)
        assert r.returncode == 0, (cmd, r.stderr[-2000:])
        u1 = resource.getrusage(resource.RUSAGE_CHILDREN)
        out.append((time.time() - t, u1.ru_utime + u1.ru_stime - u0.ru_utime - u0.ru_stime, r.stdout))
    return out[warm:]


def best(ts, i=0):
    return min(x[i] for x in ts)


def spread(ts, i=0):
    return max(x[i] for x in ts) - min(x[i] for x in ts)


def timing_fields(stdout):
    line = [l for l in stdout.split("\n") if l.startswith("timing:")][-1]
    f = {k: float(v) for k, v in re.findall(r" (wall|prepare|prepare_threads|windows_per_s|steady_windows_per_s)=([0-9.e+-]+)", line)}
    return f


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=10000)
    ap.add_argument("--tool-windows", type=int, default=2000)
    ap.add_argument("--loop-windows", type=int, default=2000)
    ap.add_argument("--cap", type=int, default=16)
    ap.add_argument("--prepare-threads", default="", help="further --prepareThreads values for (3), comma-separated")
    ap.add_argument("--parent-host", default="")
    ap.add_argument("--dir", default="/tmp/hapstage_bench")
    ap.add_argument("--out", default="")
    ap.add_argument("--skip", default="", help="parts to leave out, e.g. 23")
    args = ap.parse_args()
    row = {}

    if "1" not in args.skip:
        refs, haps, pair_ref = make_batch(args.windows)
        st = torch.cuda.current_stream()
        al = hapalign.DeviceAlign(refs, haps, pair_ref, "cuda:0")
        al.launch(st)
        al.launch_variants(args.cap, st)
        got = al.variant_results()
        assert hapalign.variants_last_launch()["guard_trips"] == 0
        t_al = timed(lambda: al.launch(st), st, args.reps)
        t_va = timed(lambda: al.launch_variants(args.cap, st, fill=None), st, args.reps)
        n = len(haps)
        nv = got["summary"][:, 0]
        row.update(windows=args.windows, pairs=n, cap=args.cap, align_s=min(t_al), align_s_all=t_al, variants_s=min(t_va), variants_s_all=t_va,
                   variants_share_of_align=min(t_va) / min(t_al), variants_us_per_window=1e6 * min(t_va) / args.windows,
                   records_per_pair=float(nv.mean()), pairs_over_cap=int((nv > args.cap).sum()),
                   pairs_host_flag=int(((got["summary"][:, 3] & capi.DD_HAP_VARIANTS_HOST) != 0).sum()),
                   bytes_back_per_pair_records=16 + 16 * args.cap + 8, bytes_back_per_pair_records_used=16 + 16 * float(np.minimum(nv, args.cap).mean()) + 8,
                   bytes_back_per_pair_slice=2 * sum(map(len, haps)) / n + 8, launch=hapalign.variants_last_launch())
        del al
        torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)

    def sample(n, sub):
        d = os.path.join(args.dir, sub)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "n2_pipeline_bench.py"), "--windows", str(n), "--dir", d, "--reps", "1", "--procs", "16"],
                           capture_output=True, text=True)
        assert "generated %d windows" % n in r.stdout, r.stdout + r.stderr
        return d

    if "2" not in args.skip:
        d = sample(args.tool_windows, "tool")
        wrh, first = os.path.join(d, "wrh.txt"), os.path.join(d, "wrh_first.txt")
        subprocess.check_call([os.path.join(HOST, "dindel_haplotypes"), "--bamFile", d + "/reads.bam", "--ref", d + "/ref.fa", "--varFile", d + "/windows.txt",
                               "--outputFile", wrh, "--quiet"], env=env(), stderr=subprocess.DEVNULL)
        text = open(wrh).read()
        second = text.index("\nW ", 1) + 1
        open(first, "w").write(text[:second])
        tool = os.path.join(HOST, "dindel_hapalign")
        res = {}
        for tag, extra in (("device", []), ("host", ["--hostConvert"])):
            t0 = run_timed([tool, "--hapFile", first, "--outputFile", d + "/a_first.txt", "--quiet"] + extra, args.reps)
            t = run_timed([tool, "--hapFile", wrh, "--outputFile", d + "/a_%s.txt" % tag, "--quiet"] + extra, args.reps)
            res[tag] = dict(wall_s=best(t), wall_all=[x[0] for x in t], cpu_s=best(t, 1), startup_wall_s=best(t0), startup_cpu_s=best(t0, 1),
                            wall_less_startup_s=best(t) - best(t0), cpu_less_startup_s=best(t, 1) - best(t0, 1), wall_spread_s=spread(t))
        same = open(d + "/a_device.txt", "rb").read() == open(d + "/a_host.txt", "rb").read()
        nW = text.count("\nW ") + 1
        row.update(hapalign_windows=nW, hapalign_haplotypes=text.count("\nH "), hapalign_outputs_equal=same, hapalign=res,
                   hapalign_us_per_window_device=1e6 * res["device"]["wall_less_startup_s"] / nW,
                   hapalign_us_per_window_host=1e6 * res["host"]["wall_less_startup_s"] / nW)
        print(json.dumps({k: row[k] for k in row if k.startswith("hapalign")}), flush=True)

    if "3" not in args.skip:
        d = sample(args.loop_windows, "loop")
        n = args.loop_windows
        base = ["--bamFile", d + "/reads.bam", "--varFile", d + "/windows.txt", "--quiet", "--timing"]
        loop = {}
        configs = [("ref", []), ("ref_hostConvert", ["--hostConvert"])] + [("ref_pt%s" % p, ["--prepareThreads", p]) for p in args.prepare_threads.split(",") if p]
        for tag, extra in configs:
            t = run_timed([os.path.join(HOST, "dindel_gpu")] + base + ["--ref", d + "/ref.fa", "--outputFile", d + "/" + tag] + extra, args.reps)
            k = min(range(len(t)), key=lambda i: t[i][0])
            f = timing_fields(t[k][2])
            loop[tag] = dict(wall_s=t[k][0], wall_all=[x[0] for x in t], windows_per_s=f.get("windows_per_s"), steady_windows_per_s=f.get("steady_windows_per_s"),
                             prepare_threads=f.get("prepare_threads"), prepare_s_per_window=f.get("prepare", 0.0) / n)
        ph = args.parent_host or HOST
        conv = [] if args.parent_host else ["--hostConvert"]
        c1 = run_timed([os.path.join(ph, "dindel_haplotypes"), "--bamFile", d + "/reads.bam", "--ref", d + "/ref.fa", "--varFile", d + "/windows.txt",
                        "--outputFile", d + "/c_wrh.txt", "--quiet"], args.reps)
        c2 = run_timed([os.path.join(ph, "dindel_hapalign"), "--hapFile", d + "/c_wrh.txt", "--outputFile", d + "/c_aligned.txt", "--quiet"] + conv, args.reps)
        c3 = run_timed([os.path.join(ph, "dindel_gpu")] + base + ["--hapFile", d + "/c_aligned.txt", "--outputFile", d + "/chain"], args.reps)
        f3 = timing_fields(c3[min(range(len(c3)), key=lambda i: c3[i][0])][2])
        # the sample's own haplotype file: what a run costs that got its haplotypes for nothing
        c4 = run_timed([os.path.join(ph, "dindel_gpu")] + base + ["--hapFile", d + "/haps.txt", "--outputFile", d + "/given"], args.reps)
        f4 = timing_fields(c4[min(range(len(c4)), key=lambda i: c4[i][0])][2])
        same = open(d + "/ref.glf.txt", "rb").read() == open(d + "/chain.glf.txt", "rb").read() == open(d + "/ref_hostConvert.glf.txt", "rb").read()
        row.update(loop_windows=n, loop=loop, loop_outputs_equal_chain=same, chain_tools="parent build" if args.parent_host else "this tree, --hostConvert",
                   chain=dict(haplotypes_wall_s=best(c1), hapalign_wall_s=best(c2), gpu_hapfile_wall_s=best(c3), sum_wall_s=best(c1) + best(c2) + best(c3),
                              windows_per_s_of_sum=n / (best(c1) + best(c2) + best(c3)), gpu_hapfile_prepare_s_per_window=f3.get("prepare", 0.0) / n),
                   hapfile_alone=dict(wall_s=best(c4), windows_per_s=f4.get("windows_per_s"), steady_windows_per_s=f4.get("steady_windows_per_s"),
                                      prepare_s_per_window=f4.get("prepare", 0.0) / n))
        print(json.dumps({k: row[k] for k in ("loop", "chain", "hapfile_alone", "loop_outputs_equal_chain")}), flush=True)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(row, f, indent=1)
