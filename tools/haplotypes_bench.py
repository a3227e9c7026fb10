#!/usr/bin/env python3
"""The block table of the haplotype distribution on the device, and dindel_haplotypes end to end with it and without.
  python tools/haplotypes_bench.py [--reps 3] [--windows 10000] [--reads 200] [--tool-windows 2000] [--out FILE.json]
Reported, best of --reps after a warm-up:
  (a) the block-table launch for --windows windows of 160 reference bases x --reads reads of 100 bases (one in ten with a 2-base
      deletion or insertion, 0.5 % substitutions), between two events on a resident batch, next to the configs[1] likelihood launch
      (as many windows x 8 haplotypes x 200 reads) of the same job;
  (b) the bytes that go in and come back per window through dd_hap_blocks_compute;
  (c) the tool on a sample of tools/n2_pipeline_bench.py's generator (--tool-windows windows, 7 candidates and 200 reads each), with the
      device table and with --hostDistribution: wall and CPU seconds, a run over the sample's first window (start-up, device
      initialisation) taken off both."""
import argparse
import json
import os
import resource
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from dindel_tgi_amd import capi, hapdist, synth
from dindel_tgi_amd.device import DeviceBatch

TOOL = os.path.join(ROOT, "dindel_tgi_amd", "host", "dindel_haplotypes")


def make_batch(W, R, seed=0xB10C):
    """The arrays of hapdist.pack() for W windows x R reads, built with numpy."""
    rng = np.random.default_rng(seed)
    step, L, RL = 150, 160, 100
    g = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 2000 + step * W + 1000)]
    rs = (1000 + step * np.arange(W)).astype(np.int32)
    pos = (np.repeat(rs, R) - 60 + rng.integers(0, 160, W * R)).astype(np.int32)
    kind = rng.choice(3, W * R, p=[0.9, 0.05, 0.05])                  # 100M, 50M2D50M, 50M2I48M
    offs = np.stack([np.arange(RL), np.concatenate([np.arange(50), np.arange(52, 102)]), np.concatenate([np.arange(50), [0, 0], np.arange(50, 98)])])
    letters = g[pos[:, None] + offs[kind]]
    letters[kind == 2, 50] = ord("G"); letters[kind == 2, 51] = ord("A")
    err = rng.random(letters.shape) < 0.005
    letters[err] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(err.sum()))]
    n_ops = np.where(kind == 0, 1, 3)
    op_off = np.concatenate([[0], np.cumsum(n_ops)]).astype(np.int32)
    ops = np.zeros(int(op_off[-1]), np.uint32)
    first = op_off[:-1]
    ops[first[kind == 0]] = (100 << 4) | 0
    for k, (mid, last) in ((1, ((2 << 4) | 2, (50 << 4) | 0)), (2, ((2 << 4) | 1, (48 << 4) | 0))):
        f = first[kind == k]
        ops[f] = (50 << 4) | 0; ops[f + 1] = mid; ops[f + 2] = last
    idx = rs[:, None] + np.arange(L)
    return {"win_rs": rs, "win_ref_off": (L * np.arange(W + 1)).astype(np.int32), "ref_seq": g[idx].reshape(-1).copy(),
            "win_read_off": (R * np.arange(W + 1)).astype(np.int32), "read_pos": pos, "read_flag": np.zeros(W * R, np.int32),
            "read_op_off": op_off, "ops": ops, "read_base_off": (RL * np.arange(W * R + 1)).astype(np.int32), "bases": letters.reshape(-1).copy()}


def timed(fn, st, reps):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st); fn(); e1.record(st)
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 1e3)
    return ts


def tool_seconds(args, reps):
    """[(wall, cpu)] of `reps` runs after a warm-up run"""
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = []
    for _ in range(reps + 1):
        u0 = resource.getrusage(resource.RUSAGE_CHILDREN)
        t = time.time()
        subprocess.check_call([TOOL] + args, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        u1 = resource.getrusage(resource.RUSAGE_CHILDREN)
        out.append((time.time() - t, u1.ru_utime + u1.ru_stime - u0.ru_utime - u0.ru_stime))
    return out[1:]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=10000)
    ap.add_argument("--reads", type=int, default=200)
    ap.add_argument("--tool-windows", type=int, default=2000)
    ap.add_argument("--dir", default="/tmp/haplotypes_bench")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    W = args.windows
    st = torch.cuda.current_stream()

    a = make_batch(W, args.reads)
    dev = hapdist.DeviceBlocks(None, None, "cuda:0", packed=a)
    dev.launch(st)
    _, t = dev.results()
    status = np.bincount(t["status"][:W], minlength=4).tolist()
    t_tab = timed(lambda: dev.launch(st), st, args.reps)
    log = hapdist.last_launch()
    bytes_in = sum(int(a[k].nbytes) for k in hapdist.BATCH_FIELDS) + 3 * 4 * (W + 1)
    bytes_back = 6 * 4 * W + int(t["blocks"].nbytes + t["entries"].nbytes + t["ins_ops"].nbytes + t["ins_pos"].nbytes)
    used_back = 6 * 4 * W + 4 * int(t["n_blocks"][:W].sum()) + 8 * int(t["n_entries"][:W].sum()) + 8 * int(t["n_ins_ops"][:W].sum()) + 8 * int(t["n_ins_pos"][:W].sum())
    row = dict(windows=W, reads=args.reads, status_counts=status, table_s=min(t_tab), table_s_all=t_tab, table_us_per_window=1e6 * min(t_tab) / W,
               blocks_per_window=float(t["n_blocks"][:W].mean()), entries_per_window=float(t["n_entries"][:W].mean()),
               bytes_in_per_window=bytes_in / W, bytes_back_per_window=bytes_back / W, bytes_back_used_per_window=used_back / W, launch=log)
    del dev
    torch.cuda.empty_cache()

    pb = synth.generate(W, H=8, R=200, L=100, hap_len=120, seed=1)
    lk = DeviceBatch(pb, capi.params_cli_defaults(), "cuda:0")
    lk.launch()
    torch.cuda.synchronize()
    t_lk = timed(lk.launch, st, args.reps)
    row.update(likelihood_s=min(t_lk), likelihood_s_all=t_lk, table_share_of_likelihood=min(t_tab) / min(t_lk))
    del lk
    torch.cuda.empty_cache()
    print(json.dumps(row), flush=True)

    d = args.dir
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "n2_pipeline_bench.py"), "--windows", str(args.tool_windows), "--dir", d, "--reps", "1", "--procs", "16"],
                       capture_output=True, text=True)
    assert "generated %d windows" % args.tool_windows in r.stdout, r.stdout + r.stderr
    first = os.path.join(d, "first.txt")
    open(first, "w").write(open(os.path.join(d, "windows.txt")).readline())
    base = ["--bamFile", os.path.join(d, "reads.bam"), "--ref", os.path.join(d, "ref.fa"), "--quiet"]
    t_none = tool_seconds(base + ["--varFile", first, "--outputFile", os.path.join(d, "n.txt")], args.reps)
    t_dev = tool_seconds(base + ["--varFile", os.path.join(d, "windows.txt"), "--outputFile", os.path.join(d, "dev.txt")], args.reps)
    t_host = tool_seconds(base + ["--varFile", os.path.join(d, "windows.txt"), "--outputFile", os.path.join(d, "host.txt"), "--hostDistribution"], args.reps)
    none_host = tool_seconds(base + ["--varFile", first, "--outputFile", os.path.join(d, "n.txt"), "--hostDistribution"], args.reps)
    same = open(os.path.join(d, "dev.txt"), "rb").read() == open(os.path.join(d, "host.txt"), "rb").read()
    text = open(os.path.join(d, "dev.txt")).read()
    n = args.tool_windows
    best = lambda ts, i: min(x[i] for x in ts)
    row.update(tool_windows=n, tool_records=text.count("\nW ") + text.startswith("W "), tool_haplotypes=text.count("\nH "), outputs_equal=same,
               tool_startup_device_s=best(t_none, 0), tool_startup_host_s=best(none_host, 0), tool_device_s=best(t_dev, 0), tool_device_all=t_dev,
               tool_host_s=best(t_host, 0), tool_host_all=t_host, tool_device_cpu_s=best(t_dev, 1), tool_host_cpu_s=best(t_host, 1),
               device_us_per_window=1e6 * (best(t_dev, 0) - best(t_none, 0)) / n, host_us_per_window=1e6 * (best(t_host, 0) - best(none_host, 0)) / n)
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(row, f, indent=1)
