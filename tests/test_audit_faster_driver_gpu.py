"""dindel_gpu --faster --auditFaster N [--auditSeed S]: in every launch of the window loop N of the windows the --faster kernels compute are
recomputed by the independent shadow kernel and compared on the device.  PREFIX.glf.txt must be the bytes of the run without the flag, the
timing line must count audited windows and pairs and no mismatch, and the exit status must be 0 — also with --deviceIndelKeys,
--longWindowsFaster, --batchWindows 1, --windowByWindow and --devices 0,0; --auditInject plants one difference in front of a window's audit
(the output files stay as they are): exit status 3, the window and `ll` on stderr; --auditFaster without --faster is refused, and
--faster --audit stays refused.

The sample is the synthetic BAM of tests/test_n2_driver_gpu.py."""
import os
import re
import subprocess

import pytest

from tests.test_audit_driver_gpu import run, tag
from tests.test_n2_driver_gpu import HOST, scene  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def test_same_bytes_windows_audited_and_no_mismatch(scene):  # noqa: F811
    text, timing, _ = run(scene, "af_plain", "--faster")
    assert "audit_windows" not in timing
    got, t, stderr = run(scene, "af_on", "--faster", "--auditFaster", "4")
    assert got == text
    assert int(t["audit_windows"]) > 0 and int(t["audit_pairs"]) > 0 and int(t["audit_mismatches"]) == 0
    assert "audit" not in stderr
    assert t["launches"] == timing["launches"] and t["hpos_bytes"] == timing["hpos_bytes"]
    got, t, _ = run(scene, "af_seed", "--faster", "--auditFaster=2", "--auditSeed", "12345")
    assert got == text and int(t["audit_windows"]) > 0 and int(t["audit_mismatches"]) == 0


@pytest.mark.parametrize("extra", [("--deviceIndelKeys",), ("--longWindowsFaster",), ("--batchWindows", "1"), ("--windowByWindow",),
                                   ("--batchWindows", "2", "--devices", "0,0", "--computeThreads", "3"),
                                   ("--deviceIndelKeys", "--windowByWindow")])
def test_the_same_bytes_in_every_way_of_running(scene, extra):  # noqa: F811
    want, _t, _ = run(scene, "af_ref_" + tag(extra), "--faster", *extra)
    got, t, stderr = run(scene, "af_" + tag(extra), "--faster", "--auditFaster", "4", *extra)
    assert got == want
    assert int(t["audit_windows"]) > 0 and int(t["audit_pairs"]) > 0 and int(t["audit_mismatches"]) == 0 and "audit" not in stderr, (t, stderr[-500:])


def test_an_injected_difference_ends_the_run_with_status_3(scene):  # noqa: F811
    text, _t, _ = run(scene, "af_inj_plain", "--faster")
    got, t, stderr = run(scene, "af_inj", "--faster", "--auditFaster", "100", "--auditInject", "2", rc=3)
    assert got == text                                                   # the hook restores the value behind the audit
    assert int(t["audit_mismatches"]) == 1
    lines = [l for l in stderr.split("\n") if l.startswith("audit mismatch:")]
    left = scene["spec"][1][0]
    assert len(lines) == 1 and re.match(r"audit mismatch: window 2 tid: 20 pos: \d+ pair: 0 field: ll\[\d+\] main: 0x[0-9a-f]+ shadow: 0x[0-9a-f]+$", lines[0]), lines
    assert abs(int(re.search(r"pos: (\d+)", lines[0]).group(1)) - left) < 200
    a, b = [int(v, 16) for v in re.search(r"main: 0x([0-9a-f]+) shadow: 0x([0-9a-f]+)", lines[0]).groups()]
    assert a ^ b == 1
    assert any(l.startswith("audit: 1 difference") and "shadow kernel" in l for l in stderr.split("\n"))
    # through the redo engine and the key entry as well
    got, t, stderr = run(scene, "af_inj_wbw", "--faster", "--auditFaster", "100", "--auditInject", "2", "--windowByWindow", "--deviceIndelKeys", rc=3)
    assert got == text and int(t["audit_mismatches"]) >= 1 and "audit mismatch: window 2 " in stderr


def test_refusals(scene):  # noqa: F811
    env = dict(os.environ)
    import torch
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    base = [os.path.join(HOST, "dindel_gpu"), "--bamFile", scene["bam"], "--varFile", scene["vf"], "--hapFile", scene["hf"], "--outputFile",
            str(scene["tmp"] / "af_refused"), "--quiet"]
    r = subprocess.run(base + ["--auditFaster", "4"], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--auditFaster needs --faster" in r.stderr and not os.path.exists(str(scene["tmp"] / "af_refused.glf.txt"))
    r = subprocess.run(base + ["--faster", "--audit", "4"], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--audit cannot be given with --faster" in r.stderr
    r = subprocess.run(base + ["--faster", "--auditSeed", "4"], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "need --audit" in r.stderr
