"""CPU-side checks of the wide-deletion option of the C ABI (DD_OPT_WIDE_DELETIONS: maxLengthDel above 31): the header, the screen's
classes, the workspace rule, every refusal with its dd_last_error(), and the driver's command line.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from dindel_tgi_amd import capi
from dindel_tgi_amd.batch import ReadRec, Window, alloc_result, pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONG, WIDE, FLONG = capi.DD_OPT_LONG_WINDOWS, capi.DD_OPT_WIDE_DELETIONS, capi.DD_OPT_LONG_WINDOWS_FASTER


def win(hap_len, read_len):
    return Window(1000, ["A" * hap_len], [ReadRec("C" * read_len, [0.99] * read_len, 0.99, 1000)])


def params(mld):
    p = capi.params_cli_defaults()
    p.maxLengthDel = mld
    return p


def screen(lib, pb, mld, options):
    p = params(mld)
    cls = np.zeros(max(pb.n_windows, 1), np.uint8)
    mx = (C.c_int32 * 4)()
    b = pb.ctypes_batch()
    n = lib.dd_screen_windows_ex(C.byref(p), C.byref(b), options, cls.ctypes.data_as(capi.c_u8p), C.byref(mx))
    return n, list(cls[:pb.n_windows]), list(mx)


@pytest.fixture(scope="module")
def lib():
    return capi.load()


@pytest.fixture(scope="module")
def batch():
    # ordinary, 575 bp (long at maxLengthDel >= 12), 900 bp, an empty read, a 5,000-bp haplotype, a 4,096-bp read, a 4,097-bp read
    return pack([win(120, 100), win(575, 100), win(900, 150), Window(1000, ["A" * 200], [ReadRec("", [], 0.99, 1000)]), win(5000, 100),
                 win(100, 4096), win(100, 4097)])


def test_header_compiles_as_c99_and_capi_mirrors_it(lib, tmp_path):
    assert lib.dd_abi_version() == capi.ABI_VERSION == 13
    src = tmp_path / "use_wide.c"
    src.write_text('#include <stdio.h>\n#include "dindel_hmm.h"\n'
                   'int main(void) {\n'
                   '  dd_params p; dd_params_cli_defaults(&p); p.maxLengthDel = 40;\n'
                   '  printf("%d %u %d %d %d\\n", DD_ABI_VERSION, DD_OPT_WIDE_DELETIONS, DD_WIDE_MAX_LENGTH_DEL, DD_LONG_LOG_WIDE, DD_MAX_LENGTH_DEL);\n'
                   '  return dd_workspace_bytes_wide(&p, NULL) == 0 && dd_launch_device_wide(&p, NULL, NULL, NULL, 0, NULL) == DD_ERR_INVALID &&\n'
                   '         dd_launch_device_faster_ex(&p, NULL, NULL, NULL, 8u) == DD_ERR_INVALID &&\n'
                   '         dd_build_tables_ex(&p, NULL, 0, NULL, 0, NULL, 8u) == DD_ERR_INVALID ? 0 : 1;\n}\n')
    exe = tmp_path / "use_wide"
    libdir = os.path.join(ROOT, "dindel_tgi_amd", "csrc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", libdir, "-ldindel_hmm", "-Wl,-rpath," + libdir, "-o", str(exe)])
    import torch
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.check_output([str(exe)], env=env).decode().split()
    assert out == ["13", str(capi.DD_OPT_WIDE_DELETIONS), str(capi.DD_WIDE_MAX_LENGTH_DEL), str(capi.DD_LONG_LOG_WIDE), str(capi.DD_MAX_LENGTH_DEL)]
    assert (capi.DD_OPT_WIDE_DELETIONS, capi.DD_WIDE_MAX_LENGTH_DEL, capi.DD_MAX_LENGTH_DEL) == (4, 2 ** 31 - 3, 31)
    for name in ("dd_build_tables_ex", "dd_workspace_bytes_wide", "dd_launch_device_wide", "dd_launch_device_faster_ex"):
        assert name in capi.EXPORTS and getattr(lib, name)


def test_screen_classes(lib, batch):
    # without the bit: as today, the whole call is refused
    n, _cls, _mx = screen(lib, batch, 40, LONG)
    assert n == capi.DD_ERR_UNSUPPORTED and capi.last_error() == "maxLengthDel outside [0,31]"
    # with both bits: every window within the long limits is DD_WIN_LONG, the empty read and the over-limit shapes stay unsupported
    n, cls, mx = screen(lib, batch, 40, LONG | WIDE)
    assert cls == [2, 2, 2, 1, 1, 2, 1] and n == 3, (n, cls)
    assert mx == [0, 0, 900, 4096]
    # at maxLengthDel <= 31 the bit changes nothing
    for mld in (5, 12, 31):
        assert screen(lib, batch, mld, LONG | WIDE) == screen(lib, batch, mld, LONG)
    assert screen(lib, batch, 31, LONG)[1] == [0, 2, 2, 1, 1, 2, 1]
    # the bit classes windows for the main model's long path only: alone, or beside the --faster model's bit, it is refused
    for opt in (WIDE, FLONG | WIDE, LONG | FLONG | WIDE):
        assert screen(lib, batch, 40, opt)[0] == capi.DD_ERR_INVALID and "DD_OPT_LONG_WINDOWS" in capi.last_error(), opt
    # the upper end of the range
    assert screen(lib, batch, capi.DD_WIDE_MAX_LENGTH_DEL, LONG | WIDE)[0] == 3
    assert screen(lib, batch, capi.DD_WIDE_MAX_LENGTH_DEL + 1, LONG | WIDE)[0] == capi.DD_ERR_INVALID and "INT32_MAX - 2" in capi.last_error()
    assert screen(lib, batch, -1, LONG | WIDE)[0] == capi.DD_ERR_UNSUPPORTED


def al256(v):
    return (v + 255) & ~255


@pytest.mark.parametrize("hap,read,K,per_cu", [(254, 300, 1, 2), (4094, 4096, 16, 1)])
def test_workspace_follows_the_layout(lib, hap, read, K, per_cu):
    """header + window list, prefix list, then per workgroup a tile of read x 256 K x 2 bytes and the 2 x 256 K doubles of beta[bMid]."""
    W = 10
    db = capi.dd_device_batch()
    db.n_windows, db.n_qual = W, 40
    db.long_max_hap_len, db.long_max_read_len = hap, read
    assert 256 * K >= hap + 2 and (K == 1 or 128 * K < hap + 2)
    off_prefix = al256(256 + 4 * W)
    off_tiles = al256(off_prefix + 8 * (W + 1))
    for wide in (False, True):
        stash = al256(read * 256 * K * (2 if wide else 1))
        tile = stash + 16 * 256 * K
        grid = max(1, min(256 * per_cu, (capi.DD_LONG_WS_BUDGET - off_tiles) // tile))
        p = params(40 if wide else 31)
        got = lib.dd_workspace_bytes_wide(C.byref(p), C.byref(db))
        assert got == off_tiles + grid * tile, (wide, got, grid, tile)
        assert got <= capi.DD_LONG_WS_BUDGET
        if not wide:
            assert got == lib.dd_workspace_bytes_long(C.byref(p), C.byref(db))            # maxLengthDel <= 31: the long launch's
    if K == 16:
        assert stash == 32 << 20                                                      # the maximum shape: 32 MiB + stash per workgroup
    p = params(40)
    assert lib.dd_workspace_bytes_long(C.byref(p), C.byref(db)) > 0                       # (that entry never looked at the params)
    assert lib.dd_workspace_bytes_wide(C.byref(params(capi.DD_WIDE_MAX_LENGTH_DEL + 1)), C.byref(db)) == 0
    db.long_max_hap_len = 4095
    assert lib.dd_workspace_bytes_wide(C.byref(p), C.byref(db)) == 0


def test_refusals_and_their_messages(lib, batch):
    pb = pack([win(120, 100)])
    b = pb.ctypes_batch()
    _arrs, res = alloc_result(pb)
    p = params(40)
    # host-pointer entries, main model
    assert lib.dd_compute_likelihoods(C.byref(p), C.byref(b), C.byref(res), 0) == capi.DD_ERR_UNSUPPORTED
    assert lib.dd_compute_likelihoods_ex(C.byref(p), C.byref(b), C.byref(res), 0, LONG) == capi.DD_ERR_UNSUPPORTED
    assert capi.last_error() == "maxLengthDel outside [0,31]"
    assert lib.dd_compute_likelihoods_ex(C.byref(p), C.byref(b), C.byref(res), 0, WIDE) == capi.DD_ERR_INVALID
    assert "DD_OPT_LONG_WINDOWS" in capi.last_error()
    assert lib.dd_compute_likelihoods_ex(C.byref(p), C.byref(b), C.byref(res), 0, LONG | WIDE | 8) == capi.DD_ERR_INVALID
    assert capi.last_error() == "unknown option bits"
    big = params(capi.DD_WIDE_MAX_LENGTH_DEL + 1)
    assert lib.dd_compute_likelihoods_ex(C.byref(big), C.byref(b), C.byref(res), 0, LONG | WIDE) == capi.DD_ERR_INVALID
    assert "INT32_MAX - 2" in capi.last_error()
    # ... and the --faster model's
    assert lib.dd_compute_likelihoods_faster(C.byref(p), C.byref(b), C.byref(res), 0) == capi.DD_ERR_UNSUPPORTED
    assert lib.dd_compute_likelihoods_faster_ex(C.byref(p), C.byref(b), C.byref(res), 0, 0) == capi.DD_ERR_UNSUPPORTED
    assert lib.dd_compute_likelihoods_faster_ex(C.byref(p), C.byref(b), C.byref(res), 0, LONG) == capi.DD_ERR_INVALID
    assert capi.last_error() == "unknown option bits"
    # the key entry takes the bit where it is needed (maxLengthDel above 31); beside a smaller value it stays an unknown bit there
    keys = np.zeros(4, np.int16)
    p10 = params(10)
    assert lib.dd_compute_likelihoods_faster_keys(C.byref(p10), C.byref(b), C.byref(res), keys.ctypes.data_as(capi.c_i16p), 0, WIDE) == capi.DD_ERR_INVALID
    assert capi.last_error() == "unknown option bits"
    assert lib.dd_compute_likelihoods_faster_keys(C.byref(p), C.byref(b), C.byref(res), keys.ctypes.data_as(capi.c_i16p), 0, WIDE | LONG) == capi.DD_ERR_INVALID
    assert lib.dd_compute_likelihoods_faster_keys(C.byref(p), C.byref(b), C.byref(res), keys.ctypes.data_as(capi.c_i16p), 0, 0) == capi.DD_ERR_UNSUPPORTED
    assert lib.dd_compute_likelihoods_faster_keys(C.byref(p), C.byref(b), C.byref(res), keys.ctypes.data_as(capi.c_i16p), 1 << 20, WIDE) == capi.DD_ERR_NO_DEVICE
    # the audits keep refusing the value, with or without the bit
    rep = capi.audit_report_buffer(4)
    rc = lib.dd_compute_likelihoods_audit(C.byref(p), C.byref(b), C.byref(res), 0, LONG | WIDE, 0, 1, rep.ctypes.data_as(C.c_void_p), 4)
    assert rc == capi.DD_ERR_INVALID and "unknown option bits" in capi.last_error()
    rc = lib.dd_compute_likelihoods_audit(C.byref(p), C.byref(b), C.byref(res), 0, LONG, 0, 1, rep.ctypes.data_as(C.c_void_p), 4)
    assert rc == capi.DD_ERR_UNSUPPORTED
    with pytest.raises(RuntimeError, match="maxLengthDel outside"):
        capi.AuditSample(p, pb, 1)
    # tables: the plain entry as today, the _ex entry with the bit; the tables themselves do not depend on the value
    hb = b
    t40, t31 = np.zeros(capi.DD_TABLE_DOUBLES), np.zeros(capi.DD_TABLE_DOUBLES)
    assert lib.dd_build_tables(C.byref(p), hb.qual_table, hb.n_qual, hb.mapq_table, hb.n_mapq, t40.ctypes.data_as(capi.c_f64p)) == capi.DD_ERR_UNSUPPORTED
    assert lib.dd_build_tables_ex(C.byref(p), hb.qual_table, hb.n_qual, hb.mapq_table, hb.n_mapq, t40.ctypes.data_as(capi.c_f64p), 0) == capi.DD_ERR_UNSUPPORTED
    n40 = lib.dd_build_tables_ex(C.byref(p), hb.qual_table, hb.n_qual, hb.mapq_table, hb.n_mapq, t40.ctypes.data_as(capi.c_f64p), WIDE)
    p31 = params(31)
    n31 = lib.dd_build_tables(C.byref(p31), hb.qual_table, hb.n_qual, hb.mapq_table, hb.n_mapq, t31.ctypes.data_as(capi.c_f64p))
    assert n40 == n31 > 0 and t40.tobytes() == t31.tobytes()
    # device-pointer entries: the checks in front of any device work
    db, dr = capi.dd_device_batch(), capi.dd_device_result()
    assert lib.dd_launch_device_wide(C.byref(big), C.byref(db), C.byref(dr), None, 0, None) == capi.DD_ERR_INVALID
    assert "INT32_MAX - 2" in capi.last_error()
    assert lib.dd_launch_device_wide(C.byref(p), C.byref(db), C.byref(dr), None, 0, None) == capi.DD_ERR_INVALID
    assert capi.last_error() == "ll and status outputs are required"
    assert lib.dd_launch_device_long(C.byref(p), C.byref(db), C.byref(dr), None, 0, None) == capi.DD_ERR_UNSUPPORTED
    assert lib.dd_launch_device(C.byref(p), C.byref(db), C.byref(dr), None, 0, None) == capi.DD_ERR_UNSUPPORTED
    assert lib.dd_launch_device_faster(C.byref(p), C.byref(db), C.byref(dr), None) == capi.DD_ERR_UNSUPPORTED
    assert lib.dd_launch_device_faster_ex(C.byref(p), C.byref(db), C.byref(dr), None, 0) == capi.DD_ERR_UNSUPPORTED
    assert lib.dd_launch_device_faster_ex(C.byref(p), C.byref(db), C.byref(dr), None, LONG) == capi.DD_ERR_INVALID
    assert "DD_OPT_WIDE_DELETIONS" in capi.last_error()
    assert lib.dd_launch_device_faster_ex(C.byref(p), C.byref(db), C.byref(dr), None, WIDE) == capi.DD_ERR_INVALID
    assert capi.last_error() == "ll and status outputs are required"                     # (past the parameter check)


def test_no_device_from_the_host_pointer_entry(lib):
    """The wide call passes every check of its arguments and ends where the device is first needed: DD_ERR_NO_DEVICE for a device ordinal
    no machine has (without a GPU: for any ordinal)."""
    pb = pack([win(120, 100), win(60, 50)])
    b = pb.ctypes_batch()
    _arrs, res = alloc_result(pb)
    p = params(40)
    nowhere = 1 << 20
    assert lib.dd_compute_likelihoods_ex(C.byref(p), C.byref(b), C.byref(res), nowhere, LONG | WIDE) == capi.DD_ERR_NO_DEVICE
    assert capi.last_error() in ("no HIP device: the likelihood path has no CPU fallback", "device ordinal out of range")
    assert lib.dd_compute_likelihoods_faster_ex(C.byref(p), C.byref(b), C.byref(res), nowhere, WIDE) == capi.DD_ERR_NO_DEVICE
    assert lib.dd_compute_likelihoods_ex(C.byref(p), C.byref(b), C.byref(res), nowhere, LONG) == capi.DD_ERR_UNSUPPORTED


def driver(*args):
    exe = os.path.join(ROOT, "dindel_tgi_amd", "host", "dindel_gpu")
    r = subprocess.run([exe, "--varFile", "w.txt", "--outputFile", "out", "--hapFile", "h.txt", "--bamFile", "r.bam", *args],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    return r.returncode, r.stderr.decode()


def test_driver_refusals():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "dindel_tgi_amd", "host")])
    rc, err = driver("--maxLengthIndel", "40")
    assert rc == 1 and "--wideDeletions" in err and "--maxLengthIndel 40" in err, (rc, err)
    rc, err = driver("--wideDeletions", "--audit", "4", "--maxLengthIndel", "40")
    assert rc == 1 and "--audit" in err and "--wideDeletions" in err and "same kernel" in err, (rc, err)
    rc, err = driver("--wideDeletions", "--faster", "--auditFaster", "4", "--maxLengthIndel", "32")
    assert rc == 1 and "--auditFaster" in err, (rc, err)
    help_text = subprocess.run([os.path.join(ROOT, "dindel_tgi_amd", "host", "dindel_gpu"), "--help"], stdout=subprocess.PIPE, timeout=60).stdout.decode()
    assert "[--wideDeletions]" in help_text
