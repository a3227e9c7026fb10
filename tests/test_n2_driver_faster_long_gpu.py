"""GPU: `dindel_gpu --faster --longWindowsFaster` end to end, on the scene of test_n2_driver_long_gpu.py (a heterozygous 2-bp deletion in a
window whose reference haplotype is 801 bp, between two ordinary windows).  With the flag the long window is called and its `qual` equals a
recomputation from the ORACLE's --faster log-likelihoods of the same reads; every other line of the .glf.txt is byte-identical to
`--faster` alone; --windowByWindow gives the same lines; without --faster the flag changes nothing."""
import ctypes as C
import json
import math

import pytest

from dindel_tgi_amd import capi, hostlib
from tests import _oracle
from tests.test_glf_vcf_cpu import GLF_COLUMNS
from tests.test_n2_driver_long_gpu import add_logs, run_driver, scene  # noqa: F401  (scene: the module's fixture)

pytestmark = pytest.mark.gpu


def test_long_windows_faster_flag_calls_the_long_window(scene):  # noqa: F811
    lines_on, rows_on = run_driver(scene, "fl_on", "--faster", "--longWindowsFaster", "--batchWindows", "4")
    lines_off, rows_off = run_driver(scene, "fl_off", "--faster", "--batchWindows", "4")
    off2 = [r for r in rows_off if r["index"] == "2"]
    assert off2 and all(r["msg"].startswith("error_window_outside_the_GPU_kernel_limits") for r in off2), [r["msg"] for r in off2]

    def others(lines):
        return [l for l in lines[1:] if l and dict(zip(GLF_COLUMNS, l.split(" ")))["index"] != "2"]
    assert others(lines_on) == others(lines_off) and len(others(lines_on)) >= 4
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
    ll = [[_oracle.pair_fast(h, r[6], [1.0 - 10 ** -3.0] * len(r[6]), r[2], int(r[7]), left, p)[0].ll for r in reads] for h in haps]
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
    print("qual", row["qual"], "recomputed", "%g" % qual)
    assert row["qual"] == "%g" % qual, (row["qual"], qual)
    assert best == (0, 1) and row["glf"].startswith("0/1:")
    assert row["realigned_position"] == str(left + d) and row["num_reads"] == str(len(reads))
    # the writer's redo engine computes the long window too, with the same lines
    lines_wbw, _ = run_driver(scene, "fl_wbw", "--faster", "--longWindowsFaster", "--windowByWindow")
    assert lines_wbw == lines_on
    # without --faster the flag changes nothing
    lines_m, _ = run_driver(scene, "m_on", "--longWindowsFaster")
    lines_m0, _ = run_driver(scene, "m_off")
    assert lines_m == lines_m0
