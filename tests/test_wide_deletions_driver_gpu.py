"""GPU: `dindel_gpu --wideDeletions` end to end on the small synthetic sample of tests/test_n2_driver_gpu.py.

--maxLengthIndel 40 --wideDeletions sends every window through the long-window kernel's wide build; --maxLengthIndel 31 --longWindows is
the largest value the main kernels take.  Both complete with called (`msg=ok`) rows, and the first is byte-identical to its own
--windowByWindow run (the writer's redo engine gets the flag too).  The two runs are NOT compared with each other: at the default pFirstgLO
they usually agree, but that is no theorem."""
import os
import subprocess

import pytest

from tests.test_glf_vcf_cpu import GLF_COLUMNS
from tests.test_n2_driver_gpu import HOST, scene  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def run_driver(scene, prefix, *extra):  # noqa: F811
    import torch
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = str(scene["tmp"] / prefix)
    subprocess.run([os.path.join(HOST, "dindel_gpu"), "--bamFile", scene["bam"], "--varFile", scene["vf"], "--hapFile", scene["hf"],
                    "--outputFile", out, "--quiet", *extra], env=env, stderr=subprocess.DEVNULL, check=True, timeout=300)
    text = open(out + ".glf.txt").read()
    lines = text.split("\n")
    assert lines[0].split(" ") == GLF_COLUMNS
    return text, [dict(zip(GLF_COLUMNS, l.split(" "))) for l in lines[1:] if l]


def called(rows):
    return [r for r in rows if r["analysis_type"] == "dip.map" and r["msg"] == "ok"]


def test_wide_deletions_run_completes_and_equals_its_window_by_window_run(scene):  # noqa: F811
    text, rows = run_driver(scene, "wide40", "--maxLengthIndel", "40", "--wideDeletions")
    assert len(called(rows)) >= 4, [(r["index"], r["msg"]) for r in rows]
    # the window whose reference haplotype is 3 bp: "hapSize error." as ever (40 > 3), not a run of error_ lines for every window
    assert any(r["index"] == "5" and r["msg"].startswith("error_") for r in rows)
    assert not any(r["msg"].startswith("error_") for r in rows if r["index"] in ("1", "2", "3", "4"))
    text_wbw, _rows = run_driver(scene, "wide40wbw", "--maxLengthIndel", "40", "--wideDeletions", "--windowByWindow")
    assert text_wbw == text
    # the largest value the main kernels take, beside it (not compared with the run above)
    _text, rows31 = run_driver(scene, "long31", "--maxLengthIndel", "31", "--longWindows")
    assert len(called(rows31)) >= 4, [(r["index"], r["msg"]) for r in rows31]


def test_faster_model_only_needs_the_check_lifted(scene):  # noqa: F811
    _text, rows = run_driver(scene, "wide40f", "--maxLengthIndel", "40", "--wideDeletions", "--faster")
    assert len(called(rows)) >= 4, [(r["index"], r["msg"]) for r in rows]
