"""GPU: `dindel_gpu --longWindows` end to end.  A synthetic BAM with a heterozygous 2-bp deletion in a window whose reference haplotype is
801 bp (beyond the main kernels' 766 bp), between two ordinary windows.  With the flag the long window is called and its `qual` equals a
recomputation from the ORACLE's log-likelihoods of the same reads (the method of test_n2_driver_gpu.py); every other line of the .glf.txt is
byte-identical to a run without the flag; without the flag the long window still gets the skipped line; the writer's redo engine
(--windowByWindow) gives the same lines; with --faster the flag changes nothing."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

from dindel_tgi_amd import capi, hostlib
from tests import _bamwriter as bw
from tests import _oracle
from tests.test_glf_vcf_cpu import GLF_COLUMNS, write_fasta

pytestmark = pytest.mark.gpu
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dindel_tgi_amd", "host")
LONG_W = 800          # window [left, left + 800]: an 801-bp reference haplotype
DEL_AT = 400          # the deletion's offset in the long window


def add_logs(a, b):
    return a + math.log(1.0 + math.exp(b - a)) if a > b else b + math.log(1.0 + math.exp(a - b))


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("n2long")
    rng = np.random.default_rng(91)
    r = list(rng.choice(list("ACGT"), 12000))
    for i in range(3, len(r)):                     # no homopolymer longer than 3
        if r[i] == r[i - 1] == r[i - 2] == r[i - 3]:
            r[i] = "ACGT"[("ACGT".index(r[i]) + 1 + i % 3) % 4]
    ref = "".join(r)
    fasta = str(tmp / "ref.fa")
    write_fasta(fasta, [("20", ref)])
    # (left, width, deletion offset): an ordinary window, the long one, an ordinary window
    spec = [(4000, 120, 60), (5600, LONG_W, DEL_AT), (8000, 120, 60)]
    windows, fixture, recs = [], [], []
    rid = 0
    for wi, (left, width, d) in enumerate(spec, start=1):
        right = left + width
        hap0 = ref[left:right + 1]
        hap1 = hap0[:d] + hap0[d + 2:]
        var = "-" + hap0[d:d + 2]
        windows.append("20 %d %d %d,%s" % (left, right, left + d, var))
        ref_v = "V I %d *REF %s" % (d, " ".join([str(d)] * 8))
        ref_s = "V S %d *REF %s" % (d, " ".join([str(d)] * 8))
        v1 = "V I %d %s %d %d %d %d %d %d %d %d" % (d, var, d, d + 1, d - 1, d, d, d + 1, d - 1, d)
        a0 = "A " + " ".join(map(str, range(width + 1)))
        a1 = "A " + " ".join(map(str, list(range(d)) + list(range(d + 2, width + 1))))
        fixture += ["W %d %d %d" % (wi, left, right), "H " + hap0, a0, ref_v, ref_s, "H " + hap1, v1, ref_s, a1]
        alt = ref[:left + d] + ref[left + d + 2:]
        for _ in range(40):
            from_alt = rng.random() < 0.5
            p = int(rng.integers(left + d - 60, left + d + 15))
            if from_alt:
                cut = left + d - p
                seq = alt[p:p + 100]
                cigar = "100M" if cut <= 0 or cut >= 100 else "%dM2D%dM" % (cut, 100 - cut)
                if cut <= 0:
                    p += 2                                  # a read right of the deletion sits two bases further on the reference
            else:
                seq, cigar = ref[p:p + 100], "100M"
            s = list(seq)
            if rng.random() < 0.1:
                k = int(rng.integers(0, 100)); s[k] = "ACGT"[("ACGT".index(s[k]) + 1) % 4]
            recs.append(dict(qname="q%04d" % rid, flag=int(rng.choice([0, 16])), pos=p, mapq=60, cigar=cigar, seq="".join(s), qual=[30] * 100,
                             mtid=-1, mpos=-1, isize=0, tags={}))
            rid += 1
    recs.sort(key=lambda r: r["pos"])
    bam = str(tmp / "reads.bam")
    bw.write_bam(bam, "@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:20\tLN:12000\n", [("20", 12000)], [(0, r) for r in recs])
    vf, hf = str(tmp / "windows.txt"), str(tmp / "haps.txt")
    open(vf, "w").write("\n".join(windows) + "\n")
    open(hf, "w").write("\n".join(fixture) + "\n")
    subprocess.check_call(["make", "-s", "-C", HOST])
    return dict(tmp=tmp, ref=ref, bam=bam, vf=vf, hf=hf, spec=spec)


def run_driver(scene, prefix, *extra):
    env = dict(os.environ)
    import torch
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = str(scene["tmp"] / prefix)
    subprocess.check_call([os.path.join(HOST, "dindel_gpu"), "--bamFile", scene["bam"], "--varFile", scene["vf"], "--hapFile", scene["hf"],
                           "--outputFile", out, "--quiet", *extra], env=env, stderr=subprocess.DEVNULL)
    lines = open(out + ".glf.txt").read().split("\n")
    assert lines[0].split(" ") == GLF_COLUMNS
    return lines, [dict(zip(GLF_COLUMNS, l.split(" "))) for l in lines[1:] if l]


def test_long_windows_flag_calls_the_long_window(scene):
    lines_on, rows_on = run_driver(scene, "on", "--longWindows", "--batchWindows", "4")
    lines_off, rows_off = run_driver(scene, "off", "--batchWindows", "4")
    # without the flag: the long window gets the skipped line, as before
    off2 = [r for r in rows_off if r["index"] == "2"]
    assert off2 and all(r["msg"].startswith("error_window_outside_the_GPU_kernel_limits") for r in off2), [r["msg"] for r in off2]
    # every line of the other windows is byte-identical with and without the flag
    def others(lines):
        return [l for l in lines[1:] if l and dict(zip(GLF_COLUMNS, l.split(" ")))["index"] != "2"]
    assert others(lines_on) == others(lines_off) and len(others(lines_on)) >= 4
    # with the flag: called, qual = the oracle's recomputation
    on2 = [r for r in rows_on if r["index"] == "2"]
    dm = [r for r in on2 if r["analysis_type"] == "dip.map"]
    assert len(dm) == 1 and dm[0]["msg"] == "ok", [(r["msg"], r["analysis_type"]) for r in on2]
    left, width, d = scene["spec"][1]
    lib = hostlib.load()
    lib.ddh_get_reads_json.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_double, C.c_char_p, C.c_int]
    out = C.create_string_buffer(1 << 24)
    win = (C.c_int * 2)(left, left + width)
    prm = (C.c_int * 4)(10000, 500, 20, 0)
    assert lib.ddh_get_reads_json(scene["bam"].encode(), b"", b"20", win, 1, prm, 0.99, out, len(out)) > 0
    reads = json.loads(out.value.decode())[0]["reads"]
    hap_lines = open(scene["hf"]).read().split("\n")
    haps = [l[2:] for l in hap_lines[hap_lines.index("W 2 %d %d" % (left, left + width)):][:9] if l.startswith("H ")]
    assert len(haps) == 2 and len(haps[0]) == width + 1 > capi.DD_MAX_HAP_LEN
    p = capi.params_cli_defaults()
    ll = [[_oracle.pair(h, r[6], [1.0 - 10 ** -3.0] * len(r[6]), r[2], int(r[7]), left, p, unmapped=bool(r[5]))[0].ll for r in reads] for h in haps]
    pp = {}
    for h1, h2 in ((0, 0), (0, 1), (1, 1)):
        s = 0.0
        for i in range(len(reads)):
            s += math.log(0.5) + add_logs(ll[h1][i], ll[h2][i])
        pp[(h1, h2)] = s + (0.0 if (h1, h2) == (0, 0) else math.log(1.0 / 10000.0))
    ll_ref = pp[(0, 0)]
    best = max(((0, 1), (1, 1)), key=lambda k: pp[k])
    qual = -10.0 * (ll_ref - add_logs(pp[best], ll_ref)) / math.log(10.0)
    row = dm[0]
    assert row["qual"] == "%g" % qual, (row["qual"], qual)
    assert best == (0, 1) and row["glf"].startswith("0/1:")
    assert row["realigned_position"] == str(left + d) and row["num_reads"] == str(len(reads))
    assert row["nref_all"] == "-" + scene["ref"][left + d:left + d + 2]
    # the writer's redo engine (every window re-done one after the other) computes the long window too, with the same lines
    lines_wbw, _ = run_driver(scene, "wbw", "--longWindows", "--windowByWindow")
    assert lines_wbw == lines_on
    # --faster: the flag has no effect (the --faster model keeps skipping such windows)
    _lf, rows_f = run_driver(scene, "f_on", "--longWindows", "--faster")
    _lf0, rows_f0 = run_driver(scene, "f_off", "--faster")
    assert _lf == _lf0
