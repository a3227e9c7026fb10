#!/usr/bin/env python3
"""What an audit of the --faster model costs on a resident batch: the audit launch (dd_audit_device_faster) next to the --faster launch it
follows (tools/audit_bench.py is the main model's).
  python tools/audit_faster_bench.py [--windows 10000] [--audit 16,100] [--reps 5] [--out FILE.json]
A resident batch in the flagship shape (BASELINE.json configs[1]: --windows windows x 8 haplotypes x 200 reads of 100 bp, haplotypes of
120 bp; 50 generated windows tiled).  For every sample size of --audit: the audit launch (the shadow kernel over the sample, then the
comparison) between two events behind dd_launch_device_faster, best of --reps after a warm-up with all repetitions beside it; the likelihood
launch itself likewise; the sample's share of the batch's pairs; the audit's cost as a share of the likelihood launch; both launches'
rates in pairs per second; what the audit found (differences, pairs compared, the shadow launch's record).  With --loop-windows N the
window loop is measured too, through tools/n2_pipeline_bench.py --faster --windows N --reps 3: --parent-driver PATH (the parent commit's
dindel_gpu), this build without the flag, and this build with --auditFaster=16; the runs' lines go into the output under "window_loop"."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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


def window_loop(a):
    """tools/n2_pipeline_bench.py three times over the same files: the parent's driver (if given), this build, this build with --auditFaster=16.
    -> {case: [the bench's JSON lines of its runs]}"""
    import subprocess
    bench = [sys.executable, os.path.join(ROOT, "tools", "n2_pipeline_bench.py"), "--faster", "--windows", str(a.loop_windows), "--reps", "3", "--dir", a.loop_dir]
    cases = ([("parent", ["--driver", a.parent_driver])] if a.parent_driver else []) + [("flag_off", []), ("audit_faster_16", ["--extra=--auditFaster=16"])]
    res = {}
    for i, (name, extra) in enumerate(cases):                 # the first case writes the sample, the others reuse it
        text = subprocess.run(bench + extra + (["--keep"] if i else []), check=True, capture_output=True, text=True).stdout
        res[name] = [json.loads(l) for l in text.split("\n") if l.startswith("{") and '"windows_per_s"' in l]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=10000)
    ap.add_argument("--audit", default="16,100")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--loop-windows", type=int, default=0, help="also run the window loop over that many windows (0: not)")
    ap.add_argument("--parent-driver", default="", help="the parent commit's dindel_gpu, for the window loop's first case")
    ap.add_argument("--loop-dir", default="/tmp/audit_faster_bench_n2")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("audit_faster_bench needs a GPU")
    gen = min(a.windows, 50)
    base = synth.generate(gen, H=8, R=200, L=100, hap_len=120, seed=0x9E3779B9)
    pb = synth.tile(base, -(-a.windows // gen))
    if pb.n_windows != a.windows:
        pb = pb.slice_windows(0, a.windows)
    p = capi.params_cli_defaults()
    out = {"device": torch.cuda.get_device_name(0), "windows": pb.n_windows, "pairs": int(pb.n_pairs), "read_len": 100, "samples": []}
    for n in [int(v) for v in a.audit.split(",")]:
        dev = DeviceBatch(pb, p, "cuda:0", audit_faster=n, audit_seed=a.seed)
        st = torch.cuda.current_stream(dev.device)
        t_main = timed(st, dev.launch_faster, a.reps)
        t_audit = timed(st, dev.launch_audit_faster, a.reps)
        rep = dev.audit_faster_results()
        log = capi.audit_last_launch_faster()
        share = rep["n_pairs"] / pb.n_pairs
        main_rate, audit_rate = pb.n_pairs / min(t_main), rep["n_pairs"] / min(t_audit)    # the audit's: shadow kernel and comparison together
        out["samples"].append({"audit_windows": int(dev.audit_faster.sizes.n_windows), "audit_pairs": rep["n_pairs"], "sample_share": share,
                               "audit_launch_s": min(t_audit), "audit_launch_s_all": t_audit, "likelihood_launch_s": min(t_main),
                               "likelihood_launch_s_all": t_main, "audit_over_likelihood": min(t_audit) / min(t_main),
                               "main_pairs_per_s": main_rate, "audit_pairs_per_s": audit_rate,
                               "differences": rep["n_diff"], "shadow_launch": log, "shadow_bytes": sum(v.numel() * v.element_size() for v in dev.shadow_faster.values()),
                               "workspace_bytes": dev.audit_faster_ws_bytes})
        del dev
    if a.loop_windows > 0:
        out["window_loop"] = window_loop(a)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
