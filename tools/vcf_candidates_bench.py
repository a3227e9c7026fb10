#!/usr/bin/env python3
"""What candidates from a VCF cost: the conversion, the realignment behind it, and the stage's share of a run.
  python tools/vcf_candidates_bench.py [--records 100000] [--windows 2000] [--reps 3] [--dir /tmp/vcf_candidates_bench] [--out FILE.json]
(1) a VCF of --records indels (length 1 ... 6, every fourth inside a planted homopolymer or 2- / 3-mer repeat) on a synthetic reference of
    ten bases per record goes through the conversion inside the host library (dindel_tgi_amd.vcf_candidates.convert): microseconds per record;
(2) its output goes through `dindel_candidates --analysis realignCandidates` inside the library on the device, once with the events
    kernel and once with --hostConvert: microseconds per candidate (the HIP context is up after the warm-up; no process start in it);
(3) on the sample of tools/discover_bench.py (tools/n2_pipeline_bench.py's generator, --windows windows) `dindel_gpu --discover` runs
    alone and with --candidateVCF naming every one of the sample's own candidates again, both with --timing: the walls, the
    "discovery_seconds:" of each and the stage's share of the run.  The windows are the same either way (a site named by both sources is
    one token), so the loop does the same work and the difference is the known sites' path alone.
Timing is the best of --reps after a warm-up, with the spread (max - min).  Nothing in the loop or the kernels depends on this path, so
nothing is compared against a threshold."""
import argparse
import json
import os
import random
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from hapstage_bench import HOST, best, run_timed, spread

VCF_HEAD = '##fileformat=VCFv4.0\n##INFO=<ID=DP,Number=1,Type=Integer,Description="Total Depth">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n'


def write_fasta(path, name, seq, width=60):
    with open(path, "w") as f:
        f.write(">%s\n" % name)
        off = f.tell()
        f.write("".join(seq[i:i + width] + "\n" for i in range(0, len(seq), width)))
    open(path + ".fai", "w").write("%s\t%d\t%d\t%d\t%d\n" % (name, len(seq), off, width, width + 1))


def synthetic(records, seed=19):
    """(reference, VCF text): one record every ten bases on average, every fourth inside a planted repeat"""
    rng = random.Random(seed)
    n = 10 * records + 1000
    s = [rng.choice("ACGT") for _ in range(n)]
    lines = []
    for k in range(records):
        at = 500 + 10 * k + rng.randrange(3)
        ln = rng.randint(1, 6)
        if k % 4 == 0:
            unit = [rng.choice("ACGT"), rng.choice(["AC", "GT"]), rng.choice(["ACG", "TTG"])][k // 4 % 3]
            s[at - 4:at - 4 + 9] = list((unit * 9)[:9])
            ln = len(unit)
        lines.append((at, ln, k % 2))
    ref = "".join(s)
    out = [VCF_HEAD]
    for at, ln, is_ins in lines:
        if is_ins:
            out.append("chrS\t%d\t.\t%s\t%s\t50\tPASS\tDP=1\n" % (at, ref[at - 1], ref[at - 1] + ref[at:at + ln]))
        else:
            out.append("chrS\t%d\t.\t%s\t%s\t50\tPASS\tDP=1\n" % (at, ref[at - 1:at + ln], ref[at - 1]))
    return ref, "".join(out)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.time()
        fn()
        ts.append((time.time() - t,))
    return ts


def candidates_in_library(args):
    import ctypes as C
    from dindel_tgi_amd import hostlib
    lib = hostlib.load()
    lib.ddh_candidates_main.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p]
    argv = (C.c_char_p * (len(args) + 2))(b"dindel_candidates", *[str(a).encode() for a in args], None)
    assert lib.ddh_candidates_main(len(args) + 1, argv, None, None) == 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--windows", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default="/tmp/vcf_candidates_bench")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    d = args.dir
    os.makedirs(d, exist_ok=True)
    from dindel_tgi_amd import vcf_candidates

    # (1) the conversion
    ref, vcf_text = synthetic(args.records)
    fa, vcf, cand = d + "/synthetic.fa", d + "/synthetic.vcf", d + "/synthetic.variants.txt"
    write_fasta(fa, "chrS", ref)
    open(vcf, "w").write(vcf_text)
    t_conv = timed(lambda: vcf_candidates.convert(vcf, fa, cand), args.reps)
    written = open(cand).read().count("\n")
    assert written == args.records, written

    # (2) the realignment behind it
    base = ["--analysis", "realignCandidates", "--varFile", cand, "--ref", fa, "--quiet"]
    t_dev = timed(lambda: candidates_in_library(base + ["--outputFile", d + "/dev"]), args.reps)
    t_host = timed(lambda: candidates_in_library(base + ["--outputFile", d + "/host", "--hostConvert"]), args.reps)
    same = open(d + "/dev.variants.txt", "rb").read() == open(d + "/host.variants.txt", "rb").read()

    # (3) the stage in a run
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "n2_pipeline_bench.py"), "--windows", str(args.windows), "--dir", d, "--reps", "1", "--procs", "16"],
                       capture_output=True, text=True)
    assert "generated %d windows" % args.windows in r.stdout, r.stdout + r.stderr
    bam, sref = d + "/reads.bam", d + "/ref.fa"
    alone, known = d + "/alone", d + "/known"
    cmd = [os.path.join(HOST, "dindel_gpu"), "--discover", "--bamFile", bam, "--ref", sref, "--quiet", "--timing"]
    t_alone = run_timed(cmd + ["--outputFile", alone], args.reps)
    seqs, name = {}, None
    for line in open(sref):
        if line.startswith(">"):
            name = line[1:].split()[0]
            seqs[name] = []
        else:
            seqs[name].append(line.strip())
    seqs = {k: "".join(v) for k, v in seqs.items()}
    sites = d + "/sites.vcf"
    with open(sites, "w") as f:                        # the sample's own candidates, named again as known sites
        f.write(VCF_HEAD)
        for line in open(alone + ".variants.txt"):
            w = line.split(" #")[0].split()
            tid, pos = w[0], int(w[1])
            for v in w[2:]:
                before = seqs[tid][pos - 1]
                f.write("%s\t%d\t.\t%s\t%s\t.\tPASS\tDP=1\n" % ((tid, pos, before, before + v[1:]) if v[0] == "+" else (tid, pos, before + v[1:], before)))
    t_known = run_timed(cmd + ["--outputFile", known, "--candidateVCF", sites], args.reps)
    stage = lambda ts: [float(re.search(r"^discovery_seconds: ([0-9.e+-]+)", x[2], re.M).group(1)) for x in ts]
    s_alone, s_known = stage(t_alone), stage(t_known)
    row = dict(records=args.records, reps=args.reps,
               convert_us_per_record=1e6 * best(t_conv) / args.records, convert_s=best(t_conv), convert_spread_s=spread(t_conv),
               realign_candidates=written, realign_outputs_equal=same,
               realign_device_events_us_per_candidate=1e6 * best(t_dev) / written, realign_device_events_s=best(t_dev), realign_device_events_spread_s=spread(t_dev),
               realign_host_convert_us_per_candidate=1e6 * best(t_host) / written, realign_host_convert_s=best(t_host), realign_host_convert_spread_s=spread(t_host),
               windows_in_sample=args.windows, known_sites=open(sites).read().count("\n") - 3,
               window_lines_alone=open(alone + ".windows.txt").read().count("\n"), window_lines_known=open(known + ".windows.txt").read().count("\n"),
               glf_equal=open(alone + ".glf.txt", "rb").read() == open(known + ".glf.txt", "rb").read(),
               discover_alone=dict(wall_s=best(t_alone), wall_all=[x[0] for x in t_alone], spread_s=spread(t_alone), stage_s=min(s_alone), stage_all=s_alone,
                                   stage_share=min(s_alone) / best(t_alone)),
               discover_known_sites=dict(wall_s=best(t_known), wall_all=[x[0] for x in t_known], spread_s=spread(t_known), stage_s=min(s_known), stage_all=s_known,
                                         stage_share=min(s_known) / best(t_known)),
               known_sites_path_s=min(s_known) - min(s_alone))
    print(json.dumps(row))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(row, open(args.out, "w"), indent=1, sort_keys=True)
        open(args.out, "a").write("\n")
