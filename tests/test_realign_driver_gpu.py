"""dindel_gpu --doPooled --outputRealignedBAM --deviceRealign: the device picks each read's haplotype by the pooled rule and only that pair's
CIGAR comes back.  The files must be the bytes of the run without the flag and of the run with --deviceCigars; no alignment comes back, and
at the default cap no read goes through the host.

The scene is the three-pool scene of tests/test_pooled_outputs_driver_gpu.py, regenerated here: two computed windows, one skipped for a
short haplotype, and one whose variant haplotype lacks its A record, so that getCIGAR throws behind the window's pooled lines.  The CPU
oracle's CIGARs of the chosen pairs say, before any run, that no read of the sample has more than 8 operations and how many have more than
one — the reads a cap of 1 sends through the host."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from dindel_tgi_amd import capi, hostlib
from tests import _bamwriter as bw
from tests import _cigar_cases as cc
from tests import _oracle
from tests.test_glf_vcf_cpu import GLF_COLUMNS
from tests.test_n2_pools_cpu import DRIVER, _env

pytestmark = pytest.mark.gpu
HOST = os.path.dirname(DRIVER)
N_REF = 12000


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("realigndrv")
    rng = np.random.default_rng(2103)
    ref = "".join(rng.choice(list("ACGT"), N_REF))
    spec = [(5000, "planted"), (5400, "pool2_empty"), (5800, "short"), (6200, "no_a_record")]
    windows, fixture, recs, hap_ref = [], [], [[], [], []], {}
    rid = 0
    for wi, (left, kind) in enumerate(spec, start=1):
        right = left + 120
        hap0 = ref[left:right + 1]
        alt = ref[:left + 60] + ref[left + 62:]
        hap1 = hap0[:60] + hap0[62:]
        var = "-" + hap0[60:62]
        windows.append("20 %d %d %d,%s" % (left, right, left + 60, var))
        v1 = "V I 60 %s 60 61 59 60 60 61 59 60" % var
        hap_ref[wi] = [list(range(121)), list(range(60)) + list(range(62, 121))]           # A records: the haplotype bases' reference offsets
        a0, a1 = ("A " + " ".join(map(str, h)) for h in hap_ref[wi])
        if kind == "short":
            fixture += ["W %d %d %d" % (wi, left, right), "H ACG", "V I 60 *REF 60 60 60 60 60 60 60 60", "H " + hap1, v1]
        else:
            fixture += ["W %d %d %d" % (wi, left, right), "H " + hap0, a0, "V I 60 *REF 60 60 60 60 60 60 60 60", "H " + hap1, v1] + ([a1] if kind != "no_a_record" else [])
        for pool in range(3):
            if kind == "pool2_empty" and pool == 2:
                continue
            for _ in range(14 if pool else 24):
                from_alt = pool == 0 and rng.random() < 0.5
                p = int(rng.integers(left - 30, left + 45))
                cut = left + 60 - p
                seq, cigar = (alt[p:p + 100], "%dM2D%dM" % (cut, 100 - cut)) if from_alt else (ref[p:p + 100], "100M")
                recs[pool].append(dict(qname="q%04d" % rid, flag=int(rng.choice([0, 16])), pos=p, mapq=int(rng.choice([40, 50, 60])), cigar=cigar, seq=seq, qual=[30] * 100,
                                       mtid=-1, mpos=-1, isize=0, tags={}))
                rid += 1
    paths = []
    for pool in range(3):
        recs[pool].sort(key=lambda r: r["pos"])
        paths.append(str(tmp / ("pool%d.bam" % pool)))
        bw.write_bam(paths[-1], "@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:20\tLN:%d\n" % N_REF, [("20", N_REF)], [(0, r) for r in recs[pool]])
    lst, vf, hf = str(tmp / "bams.txt"), str(tmp / "windows.txt"), str(tmp / "haps.txt")
    open(lst, "w").write("\n".join(paths) + "\n")
    open(vf, "w").write("\n".join(windows) + "\n")
    open(hf, "w").write("\n".join(fixture) + "\n")
    subprocess.check_call(["make", "-s", "-C", HOST])
    s = dict(tmp=tmp, ref=ref, paths=paths, list=lst, vf=vf, hf=hf, spec=spec, hap_ref=hap_ref)
    s["over_one"] = oracle_operation_counts(s)
    return s


def oracle_operation_counts(scene):
    """The CPU oracle on the reads each computed window selected: per read on a haplotype, getCIGAR (the host's, through its C hook) of its
    alignment to the first haplotype with the largest log-likelihood.  Checks that none has more than 8 operations; returns how many have
    more than one."""
    lib = hostlib.load()
    lib.ddh_get_reads_pools_json.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_double, C.c_char_p,
                                             C.c_int, C.c_char_p, C.c_int]
    n = len(scene["spec"])
    win = (C.c_int * (2 * n))(*[x for left, _ in scene["spec"] for x in (left, left + 120)])
    prm = (C.c_int * 4)(10000, 500, 20, 0)
    out = C.create_string_buffer(1 << 24)
    assert lib.ddh_get_reads_pools_json("\n".join(scene["paths"]).encode(), b"", b"20", win, n, prm, 0.99, b"", 1, out, len(out)) > 0
    selected = json.loads(out.value.decode())
    p = capi.params_cli_defaults()
    over_one = on = 0
    for wi, (left, kind) in enumerate(scene["spec"], start=1):
        if kind in ("short", "no_a_record"):               # (the latter throws at its first read on the variant haplotype: its count is dropped with it)
            continue
        hap0 = scene["ref"][left:left + 121]
        haps = [hap0, hap0[:60] + hap0[62:]]
        for r in selected[wi - 1]["reads"]:
            pairs = [_oracle.pair(h, r[6], [1.0 - 10 ** -3.0] * len(r[6]), r[2], int(r[7]), left, p, unmapped=bool(r[5])) for h in haps]
            if not any(not o.offHapHMQ for o, _ in pairs):
                continue
            best, llmax = 0, -np.inf
            for h, (o, _) in enumerate(pairs):
                if o.ll > llmax:
                    best, llmax = h, o.ll
            cig, _ref_pos = cc.host_cigar(scene["hap_ref"][wi][best], pairs[best][1])
            assert len(cig) <= 8, (wi, r[0], cig)
            on += 1
            over_one += len(cig) > 1
    assert on > 60 and 0 < over_one < on
    return over_one


def run_driver(scene, prefix, *extra):
    out = str(scene["tmp"] / prefix)
    cmd = [DRIVER, "--bamFiles", scene["list"], "--varFile", scene["vf"], "--hapFile", scene["hf"], "--outputFile", out, "--quiet", "--timing",
           "--doPooled", "--outputRealignedBAM", *extra]
    r = subprocess.run([str(c) for c in cmd], env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert r.returncode == 0, (cmd, r.stderr[-2000:])
    text = open(out + ".glf.txt").read()
    assert text.split("\n")[0].split(" ") == GLF_COLUMNS
    timing = [l for l in r.stdout.split("\n") if l.startswith("timing:")]
    assert len(timing) == 1
    d, base = os.path.split(out)
    files = {f[len(base):]: open(os.path.join(d, f), "rb").read() for f in os.listdir(d) if f.startswith(base + ".ra.")}
    return files, text, dict(re.findall(r"(\w+)=(\S+)", timing[0]))


@pytest.fixture(scope="module")
def plain(scene):
    return run_driver(scene, "plain")


def test_same_files_as_without_the_flag_and_as_with_device_cigars(scene, plain):
    files, text, timing = plain
    assert len(files) == 2 and "realign_bytes" not in timing and int(timing["hpos_bytes"]) > 0
    got_files, got_text, got = run_driver(scene, "realign", "--deviceRealign")
    assert got_files == files and got_text == text
    assert int(got["hpos_bytes"]) == 0 and int(got["cigar_bytes"]) == 0 and int(got["cigar_host_fallbacks"]) == 0 and int(got["fallback_hpos_bytes"]) == 0
    dev_files, dev_text, dev = run_driver(scene, "cigars", "--deviceCigars")
    assert dev_files == files and dev_text == text and "realign_bytes" not in dev
    # 4 cap + 16 bytes per read of the computed windows against 4 cap + 12 per pair: two haplotypes per window here
    assert int(got["realign_bytes"]) > 0 and int(got["realign_bytes"]) % 48 == 0
    assert int(dev["cigar_bytes"]) == int(got["realign_bytes"]) // 48 * 2 * 44
    # the flag wins over --deviceCigars beside it
    both_files, both_text, both = run_driver(scene, "both", "--deviceRealign", "--deviceCigars")
    assert both_files == files and both_text == text and int(both["cigar_bytes"]) == 0 and both["realign_bytes"] == got["realign_bytes"]


def test_window_without_an_alignment_writes_its_pooled_lines_then_the_skipped_line(scene, plain):
    _files, text, _ = run_driver(scene, "late", "--deviceRealign")
    assert text == plain[1]
    lines = text.split("\n")
    late = [i for i, l in enumerate(lines) if l.startswith("error_Haplotype_has_not_been_aligned!")]
    assert len(late) == 1 and lines[late[0]].split(" ")[1] == "4" and lines[late[0] - 1].split(" ")[1:3] == ["4", "singlevariant"]


def test_a_cap_of_one_sends_the_longer_cigars_through_the_host(scene, plain):
    files, text, _ = plain
    got_files, got_text, got = run_driver(scene, "cap1", "--deviceRealign", "--cigarOpsCap", "1")
    assert got_files == files and got_text == text
    assert int(got["cigar_host_fallbacks"]) == scene["over_one"] and int(got["hpos_bytes"]) == 0 and int(got["fallback_hpos_bytes"]) > 0


@pytest.mark.parametrize("extra", [("--batchWindows", "1"), ("--windowByWindow",)])
def test_batching_does_not_change_the_bytes(scene, plain, extra):
    got_files, got_text, got = run_driver(scene, "b" + extra[0][2:], "--deviceRealign", *extra)
    assert got_files == plain[0] and got_text == plain[1] and int(got["cigar_host_fallbacks"]) == 0 and int(got["hpos_bytes"]) == 0
