"""tools/check_exec_spills.py check_cmpx: a lane or DPP instruction too close behind a v_cmpx (the predicated hysteresis step of
hmm_kernel.hip lives in an asm statement, where the compiler pads no hazard) is reported; the same code one instruction later is not; and the
assembly built here is free of the pattern."""
import glob
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = """	v_add_f64 v[20:21], v[108:109], s[28:29]
	s_mov_b64 s[36:37], exec
	v_cmpx_gt_f64 vcc, v[12:13], v[20:21]
	v_mov_b64 v[108:109], v[12:13]
	v_mov_b32 v118, 2
	s_mov_b64 exec, s[36:37]
"""


def _kernel(name, tail):
    return "%s:\n%s%s\ts_endpgm\n.Lfunc_end0:\n" % (name, STEP, tail)


def test_lane_instruction_behind_cmpx(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_exec_spills as C
    f = tmp_path / "t.s"
    f.write_text(_kernel("_Zclose", "\tv_readlane_b32 s4, v9, 3\n") + _kernel("_Zpadded", "\ts_nop 0\n\tv_readlane_b32 s4, v9, 3\n") +
                 _kernel("_Zfar", "\tv_add_f64 v[2:3], v[2:3], v[4:5]\n\tv_writelane_b32 v9, s4, 3\n") +
                 _kernel("_Zdpp", "\tv_add_f64 v[2:3], v[2:3], v[4:5]\n\tv_mov_b32_dpp v1, v2 row_shr:1 row_mask:0xf bank_mask:0xf\n"))
    found = {name: C.check_cmpx(body) for name, body in C.kernels(str(f))}
    assert len(found["_Zclose"]) == 1 and "3 wait state(s), 4 needed" in found["_Zclose"][0][2]
    assert found["_Zpadded"] == [] and found["_Zfar"] == []
    assert len(found["_Zdpp"]) == 1 and "4 wait state(s), 5 needed" in found["_Zdpp"][0][2]
    built = glob.glob(os.path.join(ROOT, "dindel_tgi_amd", "csrc", "_asm", "*", "*gfx950.s"))
    if not built:
        pytest.skip("no assembly by-products here (the library was built elsewhere)")
    steps = 0
    for path in built:
        for name, body in C.kernels(path):
            assert C.check_cmpx(body) == [], (path, name)
            steps += sum("v_cmpx_gt_f64" in line for line in body)
    assert steps == 4 * 14 + 3 * 7  # the PRED_STEP builds: per position 6 steps in the right->middle sweep and 1 in the left->middle one (four K = 2 builds, three K = 1)
