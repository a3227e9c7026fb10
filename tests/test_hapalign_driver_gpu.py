"""dindel_hapalign end to end on the synthetic BAM / window / haplotype sample of tests/test_n2_driver_gpu.py: the tool's W / H / A / V
file from W / R / H records must be, byte for byte, the file tests/_hapalign_oracle.py's records make, and dindel_gpu must compute the
same calls and realigned BAMs from either.  The sample's own V / A records are not asserted: where its generator places an indel in a
repeat need not be where the alignment places it; the windows that agree are counted and printed."""
import ctypes as C
import glob
import json
import os
import subprocess

import pytest

from dindel_tgi_amd import hostlib
from tests import _hapalign_oracle as orc
from tests.test_n2_driver_gpu import HOST, run_driver, scene  # noqa: F401  (scene: the module-scoped sample)

pytestmark = pytest.mark.gpu


def fixture_windows(path, indices):
    lib = hostlib.load()
    lib.ddh_fixture_json.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.c_int, C.c_char_p, C.c_int]
    buf = C.create_string_buffer(1 << 22)
    assert lib.ddh_fixture_json(path.encode(), (C.c_int * len(indices))(*indices), len(indices), buf, len(buf)) > 0
    return json.loads(buf.value.decode())


def test_tool_output_is_the_oracle_file_and_drives_dindel_gpu(scene):  # noqa: F811
    tmp, ref = scene["tmp"], scene["ref"]
    # the sample's windows and haplotype sequences, with the block's reference sequence (getRefSeq(leftPos + 1, rightPos + 1): 1-based)
    wins, cur = [], None
    for line in open(scene["hf"]).read().split("\n"):
        f = line.split(" ")
        if f[0] == "W":
            cur = dict(index=int(f[1]), left=int(f[2]), right=int(f[3]), haps=[])
            wins.append(cur)
        elif f[0] == "H":
            cur["haps"].append(f[1])
    assert len(wins) == len(scene["spec"])
    cands, want = [], []
    for w in wins:
        block = ref[w["left"]:w["right"] + 1].upper()
        cands += ["W %d %d %d" % (w["index"], w["left"], w["right"]), "R " + block] + ["H " + h for h in w["haps"]]
        want += orc.window_records(w["index"], w["left"], w["right"], orc.window(block, w["haps"]))
    cf, of, tf = str(tmp / "cands.txt"), str(tmp / "haps_oracle.txt"), str(tmp / "haps_tool.txt")
    open(cf, "w").write("\n".join(cands) + "\n")
    open(of, "w").write("\n".join(want) + "\n")
    import torch
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    subprocess.check_call([os.path.join(HOST, "dindel_hapalign"), "--hapFile", cf, "--outputFile", tf, "--quiet", "--batchWindows", "4"], env=env)
    assert open(tf, "rb").read() == open(of, "rb").read()

    # how many windows agree with the records the sample was written with (counted, not asserted)
    idx = [w["index"] for w in wins]
    mine, theirs = fixture_windows(tf, idx), fixture_windows(scene["hf"], idx)
    print("windows whose records equal the sample's own V / A records: %d of %d" % (sum(a == b for a, b in zip(mine, theirs)), len(idx)))

    # the window loop on either file: same calls, same realigned BAMs
    outs = {}
    for name, hf in (("ho", of), ("ht", tf)):
        path, rows = run_driver(dict(scene, hf=hf), name, "--outputRealignedBAM")
        bams = sorted(glob.glob(str(tmp / name) + ".ra.*.bam"))
        outs[name] = (open(path).read(), [(os.path.basename(b)[len(name):], open(b, "rb").read()) for b in bams], rows)
    assert outs["ho"][0] == outs["ht"][0] and outs["ho"][1] == outs["ht"][1]
    assert len(outs["ht"][1]) >= 3                                      # the three windows with reads and two aligned haplotypes each
    assert any(r["msg"] == "ok" for r in outs["ht"][2])
