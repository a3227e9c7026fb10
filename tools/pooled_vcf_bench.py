#!/usr/bin/env python3
"""Wall time of dindel_pooled2vcf and dindel_pooled2glf on a generated PREFIX.glf.txt: --sites variants (default 100,000) x
--pools lines each (default 2), as `dindel_gpu --doPooled` writes them.  No GPU.  Best of --reps runs of each tool; one JSON line.

    python tools/pooled_vcf_bench.py [--sites 100000] [--pools 2] [--reps 3] [--out profiles/pooled_vcf/pooled_vcf_bench.json]"""
import argparse
import json
import os
import random
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HOST = os.path.join(ROOT, "dindel_tgi_amd", "host")
COLUMNS = ("msg index analysis_type tid lpos rpos center_position realigned_position was_candidate_in_window ref_all nref_all num_reads "
           "post_prob_variant qual est_freq logZ hapfreqs indidx msq numOffAll num_indel num_cover_forward num_cover_reverse "
           "num_unmapped_realigned var_coverage_forward var_coverage_reverse nBQT nmmBQT mLogBQ nMMLeft nMMRight glf").split()


def env():
    e = dict(os.environ)
    try:
        import torch
        e["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + e.get("LD_LIBRARY_PATH", "")
    except ImportError:
        pass
    return e


def best(cmd, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        subprocess.check_call(cmd, env=env())
        times.append(time.perf_counter() - t0)
    return min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=100000)
    ap.add_argument("--pools", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    rng = random.Random(21)
    chroms = ["1", "2", "3", "X"]
    spacing = 40
    length = (a.sites // len(chroms) + 2) * spacing + 200
    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "ref.fa")
        with open(fa, "w") as f, open(fa + ".fai", "w") as fi:
            for c in chroms:
                f.write(">%s\n" % c)
                off = f.tell()
                seq = "".join(rng.choice("ACGT") for _ in range(length))
                f.write("".join(seq[i:i + 60] + "\n" for i in range(0, length, 60)))
                fi.write("%s\t%d\t%d\t60\t61\n" % (c, length, off))
        glf = os.path.join(d, "pooled.glf.txt")
        with open(glf, "w") as f:
            f.write(" ".join(COLUMNS) + "\n")
            for s in range(a.sites):
                c, pos = chroms[s % len(chroms)], 100 + (s // len(chroms)) * spacing + rng.randrange(12)
                var = rng.choice(["-A", "-AC", "+G", "+TTT", "-ACGT"])
                prob = rng.choice(["0.99999", "0.9995", "0.93", "0.4", "0.05", "0.0001"])
                freq = "%.6g" % rng.uniform(0.01, 0.6)
                for b in range(a.pools):
                    row = dict(msg="ok", index=s + 1, analysis_type="singlevariant", tid=c, lpos=pos - 60, rpos=pos + 60, center_position=pos, realigned_position=pos,
                               was_candidate_in_window=1, nref_all=var, num_reads=rng.randrange(0, 200), post_prob_variant=prob, est_freq=freq, logZ="-1234.56789",
                               hapfreqs="0.5,0.5" if b == 0 else "NA", indidx=b, msq="58.5", num_cover_forward=rng.randrange(20), num_cover_reverse=rng.randrange(20),
                               var_coverage_forward=rng.randrange(9), var_coverage_reverse=rng.randrange(9), glf="0/0:-%.4f;0/1:-%.4f;1/1:-%.4f" % (rng.uniform(0, 90), rng.uniform(0, 9), rng.uniform(0, 90)))
                    f.write(" ".join(str(row.get(k, "NA")) for k in COLUMNS) + "\n")
        lst, bams, vcf, out = (os.path.join(d, n) for n in ("glfs.txt", "bams.txt", "calls.vcf", "called.glf.txt"))
        open(lst, "w").write(glf + "\n")
        open(bams, "w").write("".join("pool%d.bam\n" % b for b in range(a.pools)))
        t_vcf = best([os.path.join(HOST, "dindel_pooled2vcf"), "-i", lst, "-o", vcf, "-r", fa, "--numSamples", str(2 * a.pools), "--numBamFiles", str(a.pools), "--quiet"], a.reps)
        t_glf = best([os.path.join(HOST, "dindel_pooled2glf"), "-g", lst, "-c", vcf, "-o", out, "-b", bams, "--quiet"], a.reps)
        records = sum(1 for l in open(vcf) if not l.startswith("#"))
        res = dict(sites=a.sites, pools=a.pools, glf_lines=a.sites * a.pools, glf_bytes=os.path.getsize(glf), pooled2vcf_seconds=round(t_vcf, 4), pooled2glf_seconds=round(t_glf, 4),
                   vcf_records=records, vcf_pass=sum(1 for l in open(vcf) if "\tPASS\t" in l), called_glf_lines=sum(1 for _ in open(out)), reps=a.reps)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
