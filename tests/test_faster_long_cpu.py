"""CPU-side checks of the --faster model's long-window option of the C ABI (DD_OPT_LONG_WINDOWS_FASTER): the screen's classes for that
model, the workspace rule, the header.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from dindel_tgi_amd import capi
from dindel_tgi_amd.batch import pack
from tests.test_long_windows_cpu import classes, win

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FL = 2          # DD_OPT_LONG_WINDOWS_FASTER


@pytest.fixture(scope="module")
def lib():
    return capi.load()


def test_option_value():
    assert capi.DD_OPT_LONG_WINDOWS_FASTER == FL and capi.DD_OPT_LONG_WINDOWS == 1


def test_screen_classes_at_the_limits(lib):
    ws = [win(766, 100), win(767, 100), win(4094, 100), win(4095, 100),
          win(100, 1024), win(100, 1025), win(100, 4096), win(100, 4097)]
    cls, mx, n_bad = classes(lib, pack(ws), options=FL)
    assert cls == [0, 2, 2, 1, 0, 2, 2, 1] and n_bad == 2
    assert mx == [766, 1024, 4094, 4096]
    # option 0 and DD_OPT_LONG_WINDOWS: today's answers
    cls0, mx0, n0 = classes(lib, pack(ws), options=0)
    assert cls0 == [0, 1, 1, 1, 0, 1, 1, 1] and n0 == 6 and mx0 == [766, 1024, 0, 0]
    cls1, mx1, n1 = classes(lib, pack(ws), options=capi.DD_OPT_LONG_WINDOWS)
    assert cls1 == [0, 2, 2, 1, 0, 2, 2, 1] and n1 == 2 and mx1 == [766, 1024, 4094, 4096]


@pytest.mark.parametrize("mld", [0, 11, 12, 20, 31])
def test_classes_do_not_depend_on_max_length_del(lib, mld):
    """The 574-bp cap of the D = 32 build is a main-model matter: a 600-bp haplotype stays with dd_faster_kernel."""
    pb = pack([win(574, 100), win(600, 100), win(766, 100), win(767, 100)])
    cls, mx, _n = classes(lib, pb, mld=mld, options=FL)
    assert cls == [0, 0, 0, 2] and mx == [766, 100, 767, 100]
    cls1, _mx, _n = classes(lib, pb, mld=mld, options=capi.DD_OPT_LONG_WINDOWS)
    assert cls1 == ([0, 2, 2, 2] if mld >= 12 else [0, 0, 0, 2])


def test_odd_bytes_do_not_matter_to_this_model(lib):
    """27 distinct non-ACGTN haplotype bytes: the main model leaves one window without a symbol id; the --faster model compares bytes."""
    odd = [chr(c) for c in range(ord("a"), ord("a") + 27)]
    pb = pack([win(800, 100, hap_byte=b) for b in odd])
    cls, _mx, n_bad = classes(lib, pb, options=FL)
    assert cls == [2] * 27 and n_bad == 0


def test_both_bits_and_unknown_bits_are_invalid(lib):
    pb = pack([win(800, 100)])
    p = capi.params_cli_defaults()
    cls = np.zeros(1, np.uint8)
    b = pb.ctypes_batch()
    for opt in (3, 4, 6, 0x80000000):
        assert lib.dd_screen_windows_ex(C.byref(p), C.byref(b), opt, cls.ctypes.data_as(capi.c_u8p), None) == capi.DD_ERR_INVALID, opt
    # the host-pointer entries reject the other model's bit before anything else (no device needed for that)
    assert lib.dd_compute_likelihoods_ex(C.byref(p), C.byref(b), None, 0, FL) == capi.DD_ERR_INVALID
    assert lib.dd_compute_likelihoods_faster_ex(C.byref(p), C.byref(b), None, 0, capi.DD_OPT_LONG_WINDOWS) == capi.DD_ERR_INVALID
    assert lib.dd_compute_likelihoods_faster_ex(C.byref(p), C.byref(b), None, 0, 3) == capi.DD_ERR_INVALID


def ws_bytes(lib, hap, read, n_haps=1000, n_reads=100000):
    p = capi.params_cli_defaults()
    db = capi.dd_device_batch()
    db.n_windows, db.n_qual, db.n_haps, db.n_reads = 10, 40, n_haps, n_reads
    db.long_max_hap_len, db.long_max_read_len = hap, read
    return lib.dd_workspace_bytes_faster_long(C.byref(p), C.byref(db))


def test_workspace_rule(lib):
    sizes = [ws_bytes(lib, h, r) for h, r in [(767, 100), (1000, 150), (1000, 1500), (2000, 1500), (4094, 1500), (4094, 4096)]]
    assert all(0 < n <= capi.DD_FASTER_LONG_WS_BUDGET for n in sizes), sizes
    assert sizes[0] < sizes[1] < sizes[2] < sizes[3] < sizes[4]
    # the maximum shape: 16 tiles of 16 B x 4,096 rows + 2 B x 8,190 diagonals per workgroup, at least one workgroup
    assert sizes[-1] >= 16 * (16 * 4096 + 2 * 8190)
    assert ws_bytes(lib, 0, 0) == 0                                   # no long windows: nothing
    assert ws_bytes(lib, 4095, 100) == 0 and ws_bytes(lib, 100, 4097) == 0   # beyond the limits: no plan
    # grows with the pairs (items of 16 pairs of one haplotype) up to the resident grid, then not
    by_reads = [ws_bytes(lib, 2000, 150, n_haps=1, n_reads=r) for r in (1, 16, 17, 160, 1600, 16000, 160000, 1600000)]
    assert by_reads[0] == by_reads[1] < by_reads[2] < by_reads[3] < by_reads[4]
    assert by_reads[-3] == by_reads[-2] == by_reads[-1]
    one_wg = by_reads[2] - by_reads[1]
    assert (by_reads[-1] - by_reads[0]) // one_wg + 1 in (256, 512)  # one or two resident workgroups per CU


def test_abi_version_and_header_compile_as_c99(lib, tmp_path):
    assert lib.dd_abi_version() == capi.ABI_VERSION == 13
    src = tmp_path / "use_faster_long.c"
    src.write_text('#include <stdio.h>\n#include "dindel_hmm.h"\n'
                   'int main(void) {\n'
                   '  int64_t rec[DD_FASTER_LONG_LOG_FIELDS];\n'
                   '  (void)rec;\n'
                   '  printf("%d %u %d\\n", DD_ABI_VERSION, DD_OPT_LONG_WINDOWS_FASTER, (int)sizeof(dd_device_batch));\n'
                   '  return dd_screen_windows_ex(NULL, NULL, DD_OPT_LONG_WINDOWS_FASTER, NULL, NULL) == DD_ERR_INVALID &&\n'
                   '         dd_compute_likelihoods_faster_ex(NULL, NULL, NULL, 0, DD_OPT_LONG_WINDOWS_FASTER) == DD_ERR_INVALID &&\n'
                   '         dd_launch_device_faster_long(NULL, NULL, NULL, NULL, 0, NULL) == DD_ERR_INVALID &&\n'
                   '         dd_workspace_bytes_faster_long(NULL, NULL) == 0 && dd_faster_long_launch_log(NULL, 0) == 0 ? 0 : 1;\n}\n')
    exe = tmp_path / "use_faster_long"
    libdir = os.path.join(ROOT, "dindel_tgi_amd", "csrc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", libdir, "-ldindel_hmm", "-Wl,-rpath," + libdir, "-o", str(exe)])
    import torch
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.check_output([str(exe)], env=env).decode().split()
    assert out[:2] == ["13", "2"]
    assert int(out[2]) == C.sizeof(capi.dd_device_batch)
