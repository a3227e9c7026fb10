"""dindel_gpu --faster --deviceIndelKeys: the one number the window loop reads of a pair's alignment under the --faster model, the size of
its indel map, comes back from the device (2 bytes per pair) instead of the alignment.  PREFIX.glf.txt must be the bytes of the run
without the flag; no alignment comes back and no pair goes through the fallback.

The sample is the synthetic BAM of tests/test_n2_driver_gpu.py.  The CPU oracle's --faster alignments of the reads each computed window
selects say, before any run, that no pair of the sample has more than 64 keys — so the reference alone stays within the cap and a
fallback count of 0 is what must come out."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

from dindel_tgi_amd import capi, hostlib
from tests import _oracle
from tests.test_glf_vcf_cpu import GLF_COLUMNS
from tests.test_n2_driver_gpu import HOST, scene  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def oracle_key_counts(scene):  # noqa: F811
    """Per (haplotype, read) pair of the computed windows: the number of distinct keys in the indel list of the oracle's ObservationModelS."""
    lib = hostlib.load()
    lib.ddh_get_reads_json.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_double, C.c_char_p, C.c_int]
    p = capi.params_cli_defaults()
    hap_lines = open(scene["hf"]).read().split("\n")
    counts = []
    for wi, (left, _kind, _f) in enumerate(scene["spec"][:4], start=1):
        haps = [l[2:] for l in hap_lines[hap_lines.index("W %d %d %d" % (wi, left, left + 120)):][:7] if l.startswith("H ")]
        out = C.create_string_buffer(1 << 24)
        win = (C.c_int * 2)(left, left + 120)
        prm = (C.c_int * 4)(10000, 500, 20, 0)
        assert lib.ddh_get_reads_json(scene["bam"].encode(), b"", b"20", win, 1, prm, 0.99, out, len(out)) > 0
        for r in json.loads(out.value.decode())[0]["reads"]:
            for h in haps:
                o, _hp = _oracle.pair_fast(h, r[6], [1.0 - 10 ** -3.0] * len(r[6]), r[2], int(r[7]), left, p)
                assert o.n_indel < _oracle.MAXV
                counts.append(len({o.indel_pos[i] for i in range(o.n_indel)}))
    return counts


def run_driver(scene, prefix, *extra):  # noqa: F811
    env = dict(os.environ)
    import torch
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = str(scene["tmp"] / prefix)
    r = subprocess.run([os.path.join(HOST, "dindel_gpu"), "--bamFile", scene["bam"], "--varFile", scene["vf"], "--hapFile", scene["hf"], "--outputFile", out,
                        "--quiet", "--timing", *extra], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(out + ".glf.txt").read()
    assert text.split("\n")[0].split(" ") == GLF_COLUMNS
    timing = [l for l in r.stdout.split("\n") if l.startswith("timing:")]
    assert len(timing) == 1, r.stdout
    return text, dict(re.findall(r"(\w+)=(\S+)", timing[0]))


@pytest.fixture(scope="module")
def plain(scene):  # noqa: F811
    return run_driver(scene, "ik_plain", "--faster")


def test_same_bytes_no_alignments_back_and_no_fallback(scene, plain):  # noqa: F811
    counts = oracle_key_counts(scene)                                   # on the CPU, before the run
    assert len(counts) > 200 and max(counts) <= capi.DD_INDEL_KEYS_CAP and sum(c > 0 for c in counts) > 20
    text, timing = plain
    assert int(timing["hpos_bytes"]) > 0 and "indel_key_bytes" not in timing and "indel_key_fallbacks" not in timing
    assert text.count(" dip.map ") == 4
    got, t = run_driver(scene, "ik_on", "--faster", "--deviceIndelKeys")
    assert got == text
    assert int(t["hpos_bytes"]) == 0 and int(t["indel_key_fallbacks"]) == 0
    assert int(t["indel_key_bytes"]) > 0 and int(t["indel_key_bytes"]) * 100 == int(timing["hpos_bytes"])    # 2 bytes against 2 L = 200 per pair


@pytest.mark.parametrize("extra", [("--doPooled",), ("--doPooled", "--doDiploid"), ("--batchWindows", "1"), ("--windowByWindow",),
                                   ("--longWindowsFaster",), ("--batchWindows", "2", "--devices", "0,0", "--computeThreads", "3")])
def test_the_same_bytes_in_every_way_of_running(scene, plain, extra):  # noqa: F811
    ref = plain[0] if extra[0] != "--doPooled" else run_driver(scene, "ik_ref_" + "".join(e.strip("-") for e in extra), "--faster", *extra)[0]
    got, t = run_driver(scene, "ik_" + "".join(e.strip("-") for e in extra).replace(",", ""), "--faster", "--deviceIndelKeys", *extra)
    assert got == ref and int(t["hpos_bytes"]) == 0 and int(t["indel_key_fallbacks"]) == 0 and int(t["indel_key_bytes"]) > 0


def test_the_flag_without_faster_changes_nothing(scene):  # noqa: F811
    text, timing = run_driver(scene, "ik_main")
    got, t = run_driver(scene, "ik_main_flag", "--deviceIndelKeys")
    assert got == text and "indel_key_bytes" not in t and "indel_key_fallbacks" not in t
    assert t["hpos_bytes"] == timing["hpos_bytes"] and t["launches"] == timing["launches"]
