"""dindel_gpu --doPooled on a small scene with three pools (--bamFiles): a 2-bp deletion planted in half of pool 0's reads and in none of
pool 1's or pool 2's, a window where pool 2 has no reads, and a window whose likelihood step throws "hapSize error.".

The pooled lines are compared cell by cell with the Python restatement tests/_pooled_oracle.py fed with the CPU oracle's log-likelihoods
of the reads each window selected (in the manner of tests/test_n2_driver_gpu.py).  The four strand-count cells (num_cover_forward /
_reverse, var_coverage_forward / _reverse) come from the device's covered flags, which the oracle's scalars do not give: they are checked
for what must hold of them instead (tests/test_pooled_em_cpu.py checks those cells against handmade flags)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from dindel_tgi_amd import capi, hostlib
from tests import _bamwriter as bw
from tests import _oracle
from tests import _pooled_oracle as po
from tests.test_glf_vcf_cpu import GLF_COLUMNS
from tests.test_n2_pools_cpu import DRIVER, _env

pytestmark = pytest.mark.gpu
HOST = os.path.dirname(DRIVER)
FLAG_CELLS = ("num_cover_forward", "num_cover_reverse", "var_coverage_forward", "var_coverage_reverse")
N_REF = 12000


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pooled")
    rng = np.random.default_rng(2103)
    ref = "".join(rng.choice(list("ACGT"), N_REF))
    spec = [(5000, "planted"), (5400, "pool2_empty"), (5800, "short")]
    windows, fixture, recs, strand = [], [], [[], [], []], {}
    rid = 0
    for wi, (left, kind) in enumerate(spec, start=1):
        right = left + 120
        hap0 = ref[left:right + 1]
        alt = ref[:left + 60] + ref[left + 62:]
        hap1 = hap0[:60] + hap0[62:]
        var = "-" + hap0[60:62]
        windows.append("20 %d %d %d,%s" % (left, right, left + 60, var))
        v1 = "V I 60 %s 60 61 59 60 60 61 59 60" % var
        fixture += ["W %d %d %d" % (wi, left, right), "H " + ("ACG" if kind == "short" else hap0), "V I 60 *REF 60 60 60 60 60 60 60 60", "H " + hap1, v1]
        for pool in range(3):
            if kind == "pool2_empty" and pool == 2:
                continue
            for _ in range(14 if pool else 24):
                from_alt = pool == 0 and rng.random() < 0.5
                p = int(rng.integers(left - 30, left + 45))
                cut = left + 60 - p
                seq, cigar = (alt[p:p + 100], "%dM2D%dM" % (cut, 100 - cut)) if from_alt else (ref[p:p + 100], "100M")
                flag = int(rng.choice([0, 16]))
                name = "q%04d" % rid
                strand[name] = flag == 16
                recs[pool].append(dict(qname=name, flag=flag, pos=p, mapq=int(rng.choice([40, 50, 60])), cigar=cigar, seq=seq, qual=[30] * 100,
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
    return dict(tmp=tmp, ref=ref, paths=paths, list=lst, vf=vf, hf=hf, spec=spec, strand=strand)


def run_driver(scene, prefix, *extra):
    out = str(scene["tmp"] / prefix)
    r = subprocess.run([DRIVER, "--bamFiles", scene["list"], "--varFile", scene["vf"], "--hapFile", scene["hf"], "--outputFile", out, "--quiet", *extra],
                       env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(out + ".glf.txt").read()
    lines = text.split("\n")
    assert lines[0].split(" ") == GLF_COLUMNS
    return text, [dict(zip(GLF_COLUMNS, ln.split(" "))) for ln in lines[1:] if ln]


@pytest.fixture(scope="module")
def pooled_run(scene):
    return run_driver(scene, "pooled", "--doPooled")


def test_device_and_host_em_write_the_same_file(scene, pooled_run):
    assert run_driver(scene, "hostem", "--doPooled", "--hostEM")[0] == pooled_run[0]
    assert run_driver(scene, "b1", "--doPooled", "--batchWindows", "1")[0] == pooled_run[0]
    assert run_driver(scene, "wbw", "--doPooled", "--windowByWindow")[0] == pooled_run[0]


def test_one_line_per_variant_and_pool(scene, pooled_run):
    rows = pooled_run[1]
    want = []
    for wi, (left, kind) in enumerate(scene["spec"], start=1):
        if kind == "short":
            want.append((str(wi), "error_hapSize_error.", "NA", "NA"))
        else:
            want += [(str(wi), "ok", str(left + 60), str(b)) for b in range(3)]
    assert [(r["index"], r["msg"], r["realigned_position"], r["indidx"]) for r in rows] == want
    assert all(r["analysis_type"] == "singlevariant" for r in rows if r["msg"] == "ok")
    w2 = [r for r in rows if r["index"] == "2"]
    assert w2[2]["num_reads"] == "0" and w2[2]["glf"] == "0/0:0;0/1:0;1/1:0"          # pool 2 has no reads in window 2: its line is still there
    planted = [r for r in rows if r["index"] == "1"]
    assert float(planted[0]["post_prob_variant"]) > 0.5
    assert int(planted[0]["num_cover_forward"]) + int(planted[0]["num_cover_reverse"]) > 3      # pool 0 carries it
    assert planted[1]["num_cover_forward"] == planted[1]["num_cover_reverse"] == "0"              # pool 1 does not


def test_cells_match_the_restatement_on_the_oracle_likelihoods(scene, pooled_run):
    rows = pooled_run[1]
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
    for wi, (left, kind) in enumerate(scene["spec"][:2], start=1):
        reads = selected[wi - 1]["reads"]
        hap0 = scene["ref"][left:left + 121]
        haps = [hap0, hap0[:60] + hap0[62:]]
        var = "-" + hap0[60:62]
        recs = [[_oracle.pair(h, r[6], [1.0 - 10 ** -3.0] * len(r[6]), r[2], int(r[7]), left, p, unmapped=bool(r[5]))[0] for r in reads] for h in haps]
        w = dict(index=wi, tid="20", left=left, right=left + 120, cand_pos=left + 60, pools=3, cands=[(left + 60, var, -1.0)],
                 haps=[dict(filtered=0, vars={60: "*REF"}), dict(filtered=0, vars={60: var})],
                 reads=[dict(pool=int(r[8]), reverse=scene["strand"][r[0]], mapq=r[2], unmapped=bool(r[5])) for r in reads],
                 ll=[[o.ll for o in row] for row in recs], off_hap=[[bool(o.offHap) for o in row] for row in recs], covered=set(), varcov={})
        want = po.window_lines(w, "singlevariant")
        got = [r for r in rows if r["index"] == str(wi)]
        assert len(got) == len(want) == 3
        for g_row, w_row in zip(got, want):
            for col in GLF_COLUMNS:
                if col not in FLAG_CELLS:
                    assert g_row[col] == w_row.get(col, "NA"), (wi, col, g_row[col], w_row.get(col, "NA"))
            assert 0 <= int(g_row["num_cover_forward"]) + int(g_row["num_cover_reverse"]) <= int(g_row["num_reads"])
        assert len({(r["var_coverage_forward"], r["var_coverage_reverse"]) for r in got}) == 1      # the window's, on every pool's line


def test_pooled_and_diploid_lines_interleave_per_window(scene, pooled_run):
    plain_text, plain = run_driver(scene, "plain")
    both_text, both = run_driver(scene, "both", "--doPooled", "--doDiploid")
    want = []
    for wi in range(1, len(scene["spec"]) + 1):
        pooled_w = [r for r in pooled_run[1] if r["index"] == str(wi) and r["msg"] == "ok"]
        want += pooled_w + [r for r in plain if r["index"] == str(wi)]          # pooled first; a skipped window has its one line
    assert both == want
    # neither flag, or --doDiploid alone: the diploid file, byte for byte, with no pooled line in it
    assert run_driver(scene, "dip", "--doDiploid")[0] == plain_text
    assert {r["analysis_type"] for r in plain} == {"dip", "dip.map", "NA"}
    # --doDiploid takes no value: the option behind it is still read
    assert run_driver(scene, "dipq", "--doDiploid", "--batchWindows", "1")[0] == plain_text
