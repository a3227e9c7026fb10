"""dindel_gpu --audit N [--auditSeed S]: in every launch of the window loop N ordinary windows are recomputed by the long-window kernel and
compared on the device with what the main kernels wrote.  PREFIX.glf.txt must be the bytes of the run without the flag, the timing line
must count audited windows and pairs and no mismatch, and the exit status must be 0; --auditInject plants one difference in front of a
window's audit (the output files stay as they are): exit status 3, the window and `ll` on stderr; --faster --audit is refused.

The sample is the synthetic BAM of tests/test_n2_driver_gpu.py."""
import os
import re
import subprocess

import pytest

from tests.test_glf_vcf_cpu import GLF_COLUMNS
from tests.test_n2_driver_gpu import HOST, scene  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def run(scene, prefix, *extra, ref=False, rc=0):  # noqa: F811
    """-> (the .glf.txt's text, the timing line's fields, stderr)"""
    env = dict(os.environ)
    import torch
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = str(scene["tmp"] / prefix)
    haps = ["--ref", scene["fasta"]] if ref else ["--hapFile", scene["hf"]]
    r = subprocess.run([os.path.join(HOST, "dindel_gpu"), "--bamFile", scene["bam"], "--varFile", scene["vf"], *haps, "--outputFile", out,
                        "--quiet", "--timing", *extra], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == rc, (r.returncode, r.stderr[-2000:])
    text = open(out + ".glf.txt").read()
    assert text.split("\n")[0].split(" ") == GLF_COLUMNS
    timing = [l for l in r.stdout.split("\n") if l.startswith("timing:")]
    assert len(timing) == 1, r.stdout
    return text, dict(re.findall(r"(\w+)=(\S+)", timing[0])), r.stderr


def tag(extra):
    return "".join(e.strip("-") for e in extra).replace(",", "")


def test_same_bytes_windows_audited_and_no_mismatch(scene):  # noqa: F811
    text, timing, _ = run(scene, "au_plain")
    assert "audit_windows" not in timing
    got, t, stderr = run(scene, "au_on", "--audit", "4")
    assert got == text
    assert int(t["audit_windows"]) > 0 and int(t["audit_pairs"]) > 0 and int(t["audit_mismatches"]) == 0
    assert "audit" not in stderr
    assert t["launches"] == timing["launches"] and t["hpos_bytes"] == timing["hpos_bytes"]
    # another seed: the same bytes again
    got, t, _ = run(scene, "au_seed", "--audit", "2", "--auditSeed", "12345")
    assert got == text and int(t["audit_windows"]) > 0 and int(t["audit_mismatches"]) == 0


@pytest.mark.parametrize("extra", [("--doPooled",), ("--ref",), ("--batchWindows", "1"), ("--windowByWindow",), ("--longWindows",),
                                   ("--batchWindows", "2", "--devices", "0,0", "--computeThreads", "3")])
def test_the_same_bytes_in_every_way_of_running(scene, extra):  # noqa: F811
    ref = extra == ("--ref",)
    args = () if ref else extra
    want, _t, _ = run(scene, "au_ref_" + tag(extra), *args, ref=ref)
    got, t, stderr = run(scene, "au_" + tag(extra), "--audit", "4", *args, ref=ref)
    assert got == want
    assert int(t["audit_windows"]) > 0 and int(t["audit_pairs"]) > 0 and int(t["audit_mismatches"]) == 0 and "audit" not in stderr, (t, stderr[-500:])


def test_an_injected_difference_ends_the_run_with_status_3(scene):  # noqa: F811
    text, _t, _ = run(scene, "au_inj_plain")
    got, t, stderr = run(scene, "au_inj", "--audit", "100", "--auditInject", "2", rc=3)
    assert got == text                                                   # the hook restores the value behind the audit
    assert int(t["audit_mismatches"]) == 1
    lines = [l for l in stderr.split("\n") if l.startswith("audit mismatch:")]
    left = scene["spec"][1][0]
    assert len(lines) == 1 and re.match(r"audit mismatch: window 2 tid: 20 pos: \d+ pair: 0 field: ll\[\d+\] main: 0x[0-9a-f]+ long-window: 0x[0-9a-f]+$", lines[0]), lines
    assert abs(int(re.search(r"pos: (\d+)", lines[0]).group(1)) - left) < 200
    a, b = [int(v, 16) for v in re.search(r"main: 0x([0-9a-f]+) long-window: 0x([0-9a-f]+)", lines[0]).groups()]
    assert a ^ b == 1
    assert any(l.startswith("audit: 1 difference") for l in stderr.split("\n"))
    # through the redo engine as well
    got, t, stderr = run(scene, "au_inj_wbw", "--audit", "100", "--auditInject", "2", "--windowByWindow", rc=3)
    assert got == text and int(t["audit_mismatches"]) >= 1 and "audit mismatch: window 2 " in stderr


def test_audit_with_faster_is_refused(scene):  # noqa: F811
    r = subprocess.run([os.path.join(HOST, "dindel_gpu"), "--bamFile", scene["bam"], "--varFile", scene["vf"], "--hapFile", scene["hf"],
                        "--outputFile", str(scene["tmp"] / "au_refused"), "--faster", "--audit", "4"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--audit cannot be given with --faster" in r.stderr
    assert not os.path.exists(str(scene["tmp"] / "au_refused") + ".glf.txt")
    r = subprocess.run([os.path.join(HOST, "dindel_gpu"), "--bamFile", scene["bam"], "--varFile", scene["vf"], "--hapFile", scene["hf"],
                        "--outputFile", str(scene["tmp"] / "au_refused2"), "--auditInject", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "need --audit" in r.stderr
