"""CPU-side checks of the long-window option of the C ABI (DD_OPT_LONG_WINDOWS): the screen's classes, the workspace rule, the header.
No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from dindel_tgi_amd import capi
from dindel_tgi_amd.batch import ReadRec, Window, pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def win(hap_len, read_len, hap_byte="A"):
    return Window(1000, [hap_byte * hap_len], [ReadRec("C" * read_len, [0.99] * read_len, 0.99, 1000)])


def classes(lib, pb, mld=5, options=capi.DD_OPT_LONG_WINDOWS):
    p = capi.params_cli_defaults()
    p.maxLengthDel = mld
    cls = np.zeros(max(pb.n_windows, 1), np.uint8)
    mx = (C.c_int32 * 4)()
    b = pb.ctypes_batch()
    n = lib.dd_screen_windows_ex(C.byref(p), C.byref(b), options, cls.ctypes.data_as(capi.c_u8p), C.byref(mx))
    assert n >= 0, capi.last_error()
    return list(cls[:pb.n_windows]), list(mx), n


@pytest.fixture(scope="module")
def lib():
    return capi.load()


def test_screen_classes_at_the_limits(lib):
    ws = [win(766, 100), win(767, 100), win(4094, 100), win(4095, 100),
          win(100, 1024), win(100, 1025), win(100, 4096), win(100, 4097)]
    cls, mx, n_bad = classes(lib, pack(ws))
    assert cls == [0, 2, 2, 1, 0, 2, 2, 1] and n_bad == 2
    assert mx == [766, 1024, 4094, 4096]
    # without the option: the main kernels' limits, as dd_screen_windows
    cls0, mx0, n0 = classes(lib, pack(ws), options=0)
    assert cls0 == [0, 1, 1, 1, 0, 1, 1, 1] and n0 == 6 and mx0[:2] == [766, 1024] and mx0[2:] == [0, 0]


@pytest.mark.parametrize("mld,want", [(11, [0, 0]), (12, [0, 2]), (31, [0, 2])])
def test_screen_574_575_follow_max_length_del(lib, mld, want):
    """maxLengthDel >= 12 runs on the D = 32 build, which stops at 574 bp: a 575-bp haplotype goes to the long path there."""
    cls, _mx, _n = classes(lib, pack([win(574, 100), win(575, 100)]), mld=mld)
    assert cls == want
    cls0, _mx, _n = classes(lib, pack([win(574, 100), win(575, 100)]), mld=mld, options=0)
    assert cls0 == [0, 0]                       # (the plain screen does not look at params: the plain call fails such a batch instead)


def test_empty_reads_and_odd_bytes_stay_unsupported(lib):
    ws = [win(900, 100), Window(1000, ["A" * 900], [ReadRec("", [], 0.99, 1000)]), Window(1000, [""], [ReadRec("ACGT", [0.9] * 4, 0.9, 1000)])]
    cls, _mx, n_bad = classes(lib, pack(ws))
    assert cls == [2, 1, 1] and n_bad == 2
    # 27 distinct non-ACGTN haplotype bytes: the window holding the 27th (in byte order) gets no symbol id
    odd = [chr(c) for c in range(ord("a"), ord("a") + 27)]
    ws = [win(800, 100, hap_byte=b) for b in odd]
    cls, _mx, n_bad = classes(lib, pack(ws))
    assert cls == [2] * 26 + [1] and n_bad == 1


def test_options_zero_agrees_with_dd_screen_windows(lib):
    rng = np.random.default_rng(5)
    ws = [win(int(rng.integers(1, 5000)), int(rng.integers(1, 5000))) for _ in range(40)]
    pb = pack(ws)
    cls0, mx0, n0 = classes(lib, pb, options=0)
    skip = np.zeros(pb.n_windows, np.uint8)
    mx = (C.c_int32 * 2)()
    b = pb.ctypes_batch()
    n = lib.dd_screen_windows(C.byref(b), skip.ctypes.data_as(capi.c_u8p), C.byref(mx))
    assert n == n0 and list(skip) == cls0 and list(mx) == mx0[:2]
    assert lib.dd_screen_windows_ex(None, C.byref(b), 2, skip.ctypes.data_as(capi.c_u8p), None) == capi.DD_ERR_INVALID   # unknown bit


def test_workspace_grows_with_shape_and_stays_in_budget(lib):
    p = capi.params_cli_defaults()
    sizes = []
    for hap, read in [(767, 100), (1000, 150), (1000, 1500), (2000, 1500), (4094, 1500), (4094, 4096)]:
        db = capi.dd_device_batch()
        db.n_windows, db.n_qual = 10, 40
        db.long_max_hap_len, db.long_max_read_len = hap, read
        n = lib.dd_workspace_bytes_long(C.byref(p), C.byref(db))
        assert 0 < n <= capi.DD_LONG_WS_BUDGET, (hap, read, n)
        sizes.append(n)
    # grows with the shape until the budget binds; beyond, the grid shrinks instead of the call failing
    assert sizes[0] < sizes[1] < sizes[2] and min(sizes[2:]) > capi.DD_LONG_WS_BUDGET // 2
    last = sizes[-1]
    # the maximum shape still gets a grid: its tiles are 16 MiB each
    assert last >= 16 << 20
    db = capi.dd_device_batch()
    assert lib.dd_workspace_bytes_long(C.byref(p), C.byref(db)) == 0          # no long windows: nothing
    db.long_max_hap_len, db.long_max_read_len = 4095, 100
    assert lib.dd_workspace_bytes_long(C.byref(p), C.byref(db)) == 0          # beyond the limits: no plan


def test_abi_version_and_header_compile_as_c99(lib, tmp_path):
    assert lib.dd_abi_version() == capi.ABI_VERSION == 13
    src = tmp_path / "use_long.c"
    src.write_text('#include <stdio.h>\n#include "dindel_hmm.h"\n'
                   'int main(void) {\n'
                   '  dd_device_batch db; uint8_t c[1]; int32_t m[4]; int64_t rec[DD_LONG_LOG_FIELDS];\n'
                   '  (void)db; (void)c; (void)m; (void)rec;\n'
                   '  printf("%d %d %d %u %d\\n", DD_ABI_VERSION, DD_LONG_MAX_HAP_LEN, DD_LONG_MAX_READ_LEN, DD_OPT_LONG_WINDOWS,\n'
                   '         (int)sizeof(dd_device_batch));\n'
                   '  return dd_screen_windows_ex(NULL, NULL, DD_OPT_LONG_WINDOWS, NULL, NULL) == DD_ERR_INVALID &&\n'
                   '         dd_workspace_bytes_long(NULL, NULL) == 0 && dd_long_launch_log(NULL, 0) == 0 ? 0 : 1;\n}\n')
    exe = tmp_path / "use_long"
    libdir = os.path.join(ROOT, "dindel_tgi_amd", "csrc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", libdir, "-ldindel_hmm", "-Wl,-rpath," + libdir, "-o", str(exe)])
    import torch
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.check_output([str(exe)], env=env).decode().split()
    assert out[:4] == ["13", "4094", "4096", "1"]
    assert int(out[4]) == C.sizeof(capi.dd_device_batch)
