"""Real launches against tests/golden/launch_shapes.json: ten of its recipes are rebuilt and run through their entry points, and the
dd_launch_log records, dd_last_launch and dd_kernel_name must equal the recorded ones (what tests/test_launch_shape_cpu.py requires of the
shape functions alone); ll, status and the other outputs must equal the oracle's, so the arguments were filled as well as shaped."""
import numpy as np
import pytest

from dindel_tgi_amd import capi
from tests import _launch_shapes as ls
from tests import _oracle
from tests.test_gpu_parity import F64_KEYS, INT_KEYS, assert_same

pytestmark = pytest.mark.gpu
RUN = ("fold_hap61", "fold_hap62", "half_hap94", "scratch_hap120_read120", "two_waves_k3_read400", "thin_scratch_2reads", "ragged_window",
       "one_shot_two_chunks", "class_list_two_blocks", "faster_ordinary")
CASES = {c["name"]: c for c in ls.load_cases()}


def oracle_tiled(p, bases, faster):
    """The oracle's outputs for a batch made of repeated parts: each part is computed once and repeated (every array is window-major)."""
    outs = []
    for base, reps in bases:
        want = _oracle.batch(p, base, nthreads=8, faster=faster)
        n = {"hpos": base.hpos_len, "var_covered": base.var_cov_len, "var_fcov": base.var_cov_len, "onHap": base.n_reads}
        outs.append({k: np.tile(np.asarray(want[k])[:n.get(k, base.n_pairs)], reps) for k in INT_KEYS + F64_KEYS})
    return {k: np.concatenate([o[k] for o in outs]) for k in INT_KEYS + F64_KEYS}


@pytest.mark.parametrize("name", RUN)
def test_launches_equal_the_recorded_shapes(lib, name):
    case = CASES[name]
    asks, log, last, kernel, got, pb, bases = ls.run_case(lib, case)
    assert [{k: a[k] for k in ls.ASK_FIELDS} for a in case["asks"]] == asks          # the scalars the fixture was recorded with
    assert [a["record"] for a in case["asks"] if a["record"] is not None] == log
    assert last == case["last_launch"] and kernel == case["kernel_name"]
    faster = case["entry"] == "device_faster"
    assert_same(got, oracle_tiled(ls.params_of(case), bases, faster), pb)
