#!/usr/bin/env python3
"""Candidate realignment (alignCIGAR, reference GetCandidates.cpp:103-195) on the device: what it costs to get "which indels, and where"
back through the indel events of dd_align_events_kernel instead of through the per-base slice and the host conversion.
  python tools/candidates_bench.py [--reps 3] [--candidates 100000] [--out FILE.json]
The batch: --candidates indels of 1 ... 10 bases at random positions of a random reference, each in its window of 100 bases either side
(201 x ~201 pairs), one reference per pair, as host/candidates.cpp builds them.  Reported, best of --reps after a warm-up:
  (a) the alignment launch and (b) the event launch, each between two events on a resident batch;
  (c) the bytes that come back per pair either way;
  (d) the tool end to end with --hostConvert (slice back + convertHaplotypeAlignment per candidate) and (e) with the device events,
      per candidate, the wall time of a run with a single candidate (start-up, device initialisation) taken off both."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from dindel_tgi_amd import capi, hapalign

TOOL = os.path.join(ROOT, "dindel_tgi_amd", "host", "dindel_candidates")


def make_candidates(n, ref_len, seed=0xCA7D):
    rng = np.random.default_rng(seed)
    ref = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, ref_len)].tobytes().decode()
    pos = np.sort(rng.choice(np.arange(1000, ref_len - 1000), n, replace=False))
    ln = rng.integers(1, 11, n)
    ins = rng.random(n) < 0.5
    cands = []
    for p, l, i in zip(pos.tolist(), ln.tolist(), ins.tolist()):
        cands.append((p, l, "".join("ACGT"[k] for k in rng.integers(0, 4, l))) if i else (p, -l, ref[p:p + l]))
    return ref, cands


def pairs_of(ref, cands):
    refs, haps = [], []
    for p, l, s in cands:
        w = ref[p - 100:p + 101]
        refs.append(w.encode())
        haps.append((w[:100] + s + w[100:] if l > 0 else w[:100] + w[100 - l:]).encode())
    return refs, haps


def timed(fn, st, reps):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st); fn(); e1.record(st)
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 1e3)
    return ts


def tool_seconds(args, reps):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    ts = []
    for _ in range(reps + 1):                      # the first run is the warm-up
        t = time.time()
        subprocess.check_call([TOOL] + args, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        ts.append(time.time() - t)
    return ts[1:]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--candidates", type=int, default=100000)
    ap.add_argument("--events-cap", type=int, default=8)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n = args.candidates
    ref, cands = make_candidates(n, max(2000000, 30 * n))
    refs, haps = pairs_of(ref, cands)
    st = torch.cuda.current_stream()
    al = hapalign.DeviceAlign(refs, haps, list(range(n)), "cuda:0")
    al.launch(st)
    al.launch_events(args.events_cap, st)
    got, ev = al.results(), al.event_results()
    assert np.all(got["status"] == capi.DD_ALIGN_OK)
    t_al = timed(lambda: al.launch(st), st, args.reps)
    t_ev = timed(lambda: al.launch_events(args.events_cap, st, fill=None), st, args.reps)
    log, elog = hapalign.last_launch(), hapalign.events_last_launch()
    hap_bytes = int(sum(len(h) for h in haps))
    with tempfile.TemporaryDirectory() as tmp:
        fasta = os.path.join(tmp, "r.fa")
        with open(fasta, "w") as f:
            f.write(">b\n")
            off = f.tell()
            for i in range(0, len(ref), 60):
                f.write(ref[i:i + 60] + "\n")
        open(fasta + ".fai", "w").write("b\t%d\t%d\t60\t61\n" % (len(ref), off))
        vf, empty = os.path.join(tmp, "in.txt"), os.path.join(tmp, "none.txt")
        open(vf, "w").write("".join("b %d %s%s # 1\n" % (p, "+" if l > 0 else "-", s) for p, l, s in cands))
        open(empty, "w").write("b 5000 +A # 1\n")              # one candidate: the device is initialised and one launch is made
        base = ["--analysis", "realignCandidates", "--ref", fasta, "--quiet", "--eventsCap", str(args.events_cap)]
        t_none = tool_seconds(base + ["--varFile", empty, "--outputFile", os.path.join(tmp, "n")], args.reps)
        t_host = tool_seconds(base + ["--varFile", vf, "--outputFile", os.path.join(tmp, "h"), "--hostConvert"], args.reps)
        t_dev = tool_seconds(base + ["--varFile", vf, "--outputFile", os.path.join(tmp, "d")], args.reps)
        same = open(os.path.join(tmp, "h.variants.txt")).read() == open(os.path.join(tmp, "d.variants.txt")).read()
        lines = open(os.path.join(tmp, "d.variants.txt")).read().count("\n")
    row = dict(candidates=n, events_cap=args.events_cap, hap_len=[min(map(len, haps)), max(map(len, haps))], ref_len=[min(map(len, refs)), max(map(len, refs))],
               align_s=min(t_al), align_s_all=t_al, events_s=min(t_ev), events_s_all=t_ev, events_share_of_align=min(t_ev) / min(t_al),
               bytes_back_slice_per_pair=2.0 * hap_bytes / n + 8, bytes_back_events_per_pair=8.0 * args.events_cap + 12,
               pairs_over_cap=int((ev["n_events"] > args.events_cap).sum()), events_total=int(ev["n_events"].sum()),
               tool_startup_s=min(t_none), tool_host_convert_s=min(t_host), tool_host_convert_s_all=t_host, tool_device_events_s=min(t_dev),
               tool_device_events_s_all=t_dev, host_convert_us_per_candidate=1e6 * (min(t_host) - min(t_none)) / n,
               device_events_us_per_candidate=1e6 * (min(t_dev) - min(t_none)) / n, outputs_equal=same, output_lines=lines,
               launch=log, events_launch=elog)
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(row, f, indent=1)
