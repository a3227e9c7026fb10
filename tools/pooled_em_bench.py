#!/usr/bin/env python3
"""The EM launch of the pooled analysis (dd_pooled_em_device) next to dd_pooled_em_host on 16 threads.
  python tools/pooled_em_bench.py [--reps 5] [--host-threads 16] [--out FILE.json]
Two shapes, 8 sets of active variants per window (all haplotypes compatible, and the reference haplotype with each other one):
  windows  10,000 windows x 8 haplotypes x 200 reads    (80,000 slots)
  pool        200 windows x 8 haplotypes x 10,000 reads  (1,600 slots)
The ll are synthetic (no likelihood launch): a read fits the haplotype it came from and, by chance, some of the others; the rest are 12
or 30 log units worse.  Reported per shape, best of --reps after a warm-up: the launch between two events on a resident batch, the slots'
iterations, the exp / log evaluations the loop needs by its shape (2 per read, haplotype and iteration) and their rate; the host evaluation
of the first --host-windows windows on --host-threads threads, by the wall clock, scaled to the batch; and whether the two agree bit for
bit on those windows.
Then dindel_gpu --doPooled --timing on a sample of tools/n2_pipeline_bench.py's generator (--tool-windows windows of 8 haplotypes x 200
reads, one pool) against the same run with --hostEM: wall seconds, the steady rate and the compute stage's `pooled=` share from the
timing line, best of --reps after a warm-up run, and whether the two files are the same."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from dindel_tgi_amd import capi, pooled


def make_shape(W, H, R, seed):
    rng = np.random.default_rng(seed)
    origin = np.where(rng.random((W, 1, R)) < 0.8, 0, rng.integers(1, H, (W, 1, R)))
    pen = rng.choice([0.7, 12.0, 30.0], size=(W, H, R), p=[0.3, 0.4, 0.3])
    pen[np.arange(H)[None, :, None] == origin] = 0.0
    ll = (rng.uniform(-60.0, -5.0, (W, 1, R)) - pen).reshape(-1)
    who, wro = (H * np.arange(W + 1)).astype(np.int32), (R * np.arange(W + 1)).astype(np.int32)
    sets = [[1] * H] + [[1 if h in (0, k) else 0 for h in range(H)] for k in range(1, H)]
    sw = np.repeat(np.arange(W, dtype=np.int32), len(sets))
    slots = {"slot_window": sw, "slot_off": (H * np.arange(len(sw) + 1)).astype(np.int64), "compat": np.tile(np.array(sets, np.uint8).reshape(-1), W)}
    return who, wro, ll, slots


def run_shape(name, W, H, R, host_windows, reps, threads, a0, tol):
    lib = capi.load()
    dev = torch.device("cuda:0")
    who, wro, ll, slots = make_shape(W, H, R, seed=W + R)
    n, f = len(slots["slot_window"]), int(slots["slot_off"][-1])
    t = {"who": torch.from_numpy(who).to(dev), "wro": torch.from_numpy(wro).to(dev),
         "po": torch.from_numpy((H * R * np.arange(W + 1)).astype(np.int64)).to(dev), "ll": torch.from_numpy(ll).to(dev),
         "sw": torch.from_numpy(slots["slot_window"]).to(dev), "so": torch.from_numpy(slots["slot_off"]).to(dev),
         "c": torch.from_numpy(slots["compat"]).to(dev)}
    out = {"loglik": torch.zeros(n, dtype=torch.float64, device=dev), "freqs": torch.zeros(f, dtype=torch.float64, device=dev),
           "iters": torch.zeros(n, dtype=torch.int32, device=dev), "ediff": torch.zeros(n, dtype=torch.float64, device=dev)}
    db = capi.dd_device_batch()
    db.n_windows = W
    db.win_hap_off, db.win_read_off, db.win_pair_off = t["who"].data_ptr(), t["wro"].data_ptr(), t["po"].data_ptr()
    s = capi.dd_pooled_slots(n, t["sw"].data_ptr(), t["so"].data_ptr(), t["c"].data_ptr())
    r = capi.dd_pooled_result(*[out[k].data_ptr() for k in capi.POOLED_RESULT_FIELDS])
    st = torch.cuda.current_stream(dev)

    def launch():
        rc = lib.dd_pooled_em_device(C.byref(db), C.c_void_p(t["ll"].data_ptr()), C.byref(s), H, a0, tol, C.byref(r), C.c_void_p(st.cuda_stream))
        if rc != 0:
            raise RuntimeError("dd_pooled_em_device: %d %s" % (rc, capi.last_error()))
    launch()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st); launch(); e1.record(st)
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 1e3)
    got = {k: out[k].cpu().numpy() for k in out}
    evals = 2.0 * R * H * float(got["iters"].astype(np.int64).sum())
    # the host evaluation of the first windows
    hw = min(host_windows, W)
    per = n // W
    hs = {"slot_window": slots["slot_window"][:hw * per], "slot_off": slots["slot_off"][:hw * per + 1], "compat": slots["compat"][:hw * per * H]}
    hts = []
    for _ in range(2):
        t0 = time.time()
        want = pooled.em_host(who[:hw + 1], wro[:hw + 1], ll[:hw * H * R], hs, a0=a0, tol=tol, nthreads=threads)
        hts.append(time.time() - t0)
    same = all(np.array_equal(want[k], got[k][:len(want[k])]) for k in want)
    host_s = min(hts) * W / hw
    res = {"shape": name, "windows": W, "haplotypes": H, "reads": R, "slots": n, "launch_s": min(ts), "launch_s_all": ts,
           "us_per_slot": min(ts) / n * 1e6, "mean_iterations": float(got["iters"].mean()), "max_iterations": int(got["iters"].max()),
           "exp_log_evaluations": evals, "evaluations_per_s": evals / min(ts), "host_threads": threads, "host_windows": hw,
           "host_s_sample": min(hts), "host_s_scaled_to_batch": host_s, "host_over_device": host_s / min(ts), "bit_equal_on_sample": bool(same)}
    print(json.dumps(res))
    return res


def run_tool(windows, reps, directory):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "n2_pipeline_bench.py"), "--windows", str(windows), "--dir", directory, "--reps", "1", "--procs", "16"],
                       capture_output=True, text=True)
    assert "generated %d windows" % windows in r.stdout, r.stdout + r.stderr
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    base = [os.path.join(ROOT, "dindel_tgi_amd", "host", "dindel_gpu"), "--bamFile", os.path.join(directory, "reads.bam"), "--varFile", os.path.join(directory, "windows.txt"),
            "--hapFile", os.path.join(directory, "haps.txt"), "--timing", "--quiet"]
    res = {"tool_windows": windows}
    for tag, extra in (("diploid", []), ("pooled_device", ["--doPooled"]), ("pooled_host", ["--doPooled", "--hostEM"])):
        runs = []
        for _ in range(reps + 1):
            t0 = time.time()
            p = subprocess.run(base + ["--outputFile", os.path.join(directory, tag)] + extra, env=env, capture_output=True, text=True)
            wall = time.time() - t0
            assert p.returncode == 0, p.stderr[-2000:]
            line = [ln for ln in p.stdout.split("\n") if ln.startswith("timing:")][0]
            num = lambda k: float(re.search(r" %s=([0-9.eE+-]+)" % k, line).group(1)) if re.search(r" %s=" % k, line) else None
            runs.append(dict(wall=wall, steady_windows_per_s=num("steady_windows_per_s"), compute=num("compute"), pooled=num("pooled"), reduce=num("reduce")))
        res[tag] = min(runs[1:], key=lambda x: x["wall"])
        res[tag + "_walls"] = [x["wall"] for x in runs[1:]]
    res["files_equal"] = open(os.path.join(directory, "pooled_device.glf.txt"), "rb").read() == open(os.path.join(directory, "pooled_host.glf.txt"), "rb").read()
    res["pooled_lines"] = open(os.path.join(directory, "pooled_device.glf.txt")).read().count("\n") - 1
    print(json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--a0", type=float, default=0.001)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--tool-windows", type=int, default=2000)
    ap.add_argument("--dir", default="/tmp/pooled_em_bench")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pooled_em_bench needs a GPU")
    res = [run_shape("windows", 10000, 8, 200, 1000, a.reps, a.host_threads, a.a0, a.tol),
           run_shape("pool", 200, 8, 10000, 20, a.reps, a.host_threads, a.a0, a.tol)]
    tool = run_tool(a.tool_windows, a.reps, a.dir) if a.tool_windows > 0 else None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "shapes": res, "driver": tool}, f, indent=1)


if __name__ == "__main__":
    main()
