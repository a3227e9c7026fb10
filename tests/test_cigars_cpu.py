"""CPU-side checks of the device-side getCIGAR additions to the C ABI (dd_cigar_result, dd_cigars_device,
dd_compute_likelihoods_cigars): declarations, layout, validation, no CPU fallback; and that the adversarial alignments the GPU test feeds
the kernel reach every branch and every reachable throw of host/cigar.cpp.  No compute here."""
import ctypes as C
import os
import subprocess

import numpy as np

from dindel_tgi_amd import capi
from dindel_tgi_amd.batch import alloc_result
from tests import _cigar_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_compiles_as_c99_and_layout_agrees_with_ctypes(lib, tmp_path):
    src = tmp_path / "use_cigars.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dindel_hmm.h"\n'
                   'int main(void) {\n'
                   '  dd_cigar_result c; (void)c;\n'
                   '  printf("%d %d %d %d %d\\n", (int)sizeof(dd_cigar_result), (int)offsetof(dd_cigar_result, n_ops), (int)offsetof(dd_cigar_result, ops),\n'
                   '         (int)offsetof(dd_cigar_result, ref_off), (int)offsetof(dd_cigar_result, status));\n'
                   '  printf("%d %d %d %d %d %d %d %d %d %d\\n", DD_CIGAR_OK, DD_CIGAR_HAP_NOT_ALIGNED, DD_CIGAR_ERROR1, DD_CIGAR_ERROR2, DD_CIGAR_ERROR3,\n'
                   '         DD_CIGAR_ERROR4, DD_CIGAR_IMPOSSIBLE, DD_CIGAR_OVERFLOW, DD_CIGAR_NOT_COMPUTED, DD_CIGAR_DEFAULT_OPS_CAP);\n'
                   '  return dd_cigars_device(NULL, NULL, NULL, NULL, NULL, NULL, 8, NULL) == DD_ERR_INVALID &&\n'
                   '         dd_compute_likelihoods_cigars(NULL, NULL, NULL, NULL, NULL, NULL, 8, 0, 0) == DD_ERR_INVALID ? 0 : 1;\n}\n')
    exe = tmp_path / "use_cigars"
    libdir = os.path.join(ROOT, "dindel_tgi_amd", "csrc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", libdir, "-ldindel_hmm", "-Wl,-rpath," + libdir, "-o", str(exe)])
    import torch
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    lines = subprocess.check_output([str(exe)], env=env).decode().splitlines()
    T = capi.dd_cigar_result
    assert [int(v) for v in lines[0].split()] == [C.sizeof(T), T.n_ops.offset, T.ops.offset, T.ref_off.offset, T.status.offset]
    assert [int(v) for v in lines[1].split()] == [capi.DD_CIGAR_OK, capi.DD_CIGAR_HAP_NOT_ALIGNED, capi.DD_CIGAR_ERROR1, capi.DD_CIGAR_ERROR2,
                                                  capi.DD_CIGAR_ERROR3, capi.DD_CIGAR_ERROR4, capi.DD_CIGAR_IMPOSSIBLE, capi.DD_CIGAR_OVERFLOW,
                                                  capi.DD_CIGAR_NOT_COMPUTED, capi.DD_CIGAR_DEFAULT_OPS_CAP]
    # the status codes follow the order of host/cigar.cpp's throw strings
    assert [capi.CIGAR_MESSAGES[k] for k in sorted(capi.CIGAR_MESSAGES)] == ["Haplotype has not been aligned!", "Error(1)!", "Error(2)!",
                                                                              "Error(3)!", "Error(4)!", "How is this possible? (1)"]
    assert lib.dd_abi_version() == capi.ABI_VERSION


def _host_call(lib, pb, ops_cap=8, hap_ref_pos="identity", options=0, with_hpos=True):
    p = capi.params_cli_defaults()
    arrs, res = alloc_result(pb)
    if not with_hpos:
        res.hpos = None
    n = max(pb.n_pairs, 1)
    out = dict(n_ops=np.zeros(n, np.int32), ops=np.zeros((n, max(ops_cap, 1)), np.uint32), ref_off=np.zeros(n, np.int32), status=np.zeros(n, np.int32))
    cig = capi.dd_cigar_result(*[out[k].ctypes.data for k in ("n_ops", "ops", "ref_off", "status")])
    hrp = np.arange(int(pb.a["hap_seq_off"][-1]), dtype=np.int32) if isinstance(hap_ref_pos, str) else hap_ref_pos
    b = pb.ctypes_batch()
    rc = lib.dd_compute_likelihoods_cigars(C.byref(p), C.byref(b), C.byref(res), None if hrp is None else hrp.ctypes.data_as(capi.c_i32p), None,
                                           C.byref(cig), ops_cap, 0, options)
    return rc, out


def test_host_entry_validates_and_has_no_cpu_fallback(lib):
    import torch
    pb = cc.csr_batch([([30], [20, 20])])
    rc, _ = _host_call(lib, pb, ops_cap=0)
    assert rc == capi.DD_ERR_INVALID and "ops_cap" in capi.last_error()
    rc, _ = _host_call(lib, pb, ops_cap=-3)
    assert rc == capi.DD_ERR_INVALID
    rc, _ = _host_call(lib, pb, hap_ref_pos=None)
    assert rc == capi.DD_ERR_INVALID and "hap_ref_pos" in capi.last_error()
    rc, _ = _host_call(lib, pb, options=capi.DD_OPT_LONG_WINDOWS_FASTER)      # the main model's entry: only its own option bit
    assert rc == capi.DD_ERR_INVALID
    if not torch.cuda.is_available():
        for with_hpos in (True, False):                                       # r->hpos == NULL is accepted: the error is the missing device
            rc, _ = _host_call(lib, pb, with_hpos=with_hpos)
            assert rc == capi.DD_ERR_NO_DEVICE and "no CPU fallback" in capi.last_error()


def test_device_entry_validates_its_arguments(lib):
    db = capi.dd_device_batch()
    db.n_windows = db.n_haps = db.n_reads = 1
    out = capi.dd_cigar_result(8, 8, 8, 8)                                     # never dereferenced: every call below is refused first
    ok = dict(hpos=8, status=None, hrp=8, hal=None, out=C.byref(out), cap=8)
    def call(**kw):
        a = dict(ok, **kw)
        return lib.dd_cigars_device(C.byref(db), a["hpos"], a["status"], a["hrp"], a["hal"], a["out"], a["cap"], None)
    assert call(cap=0) == capi.DD_ERR_INVALID and "ops_cap" in capi.last_error()
    assert call(hrp=None) == capi.DD_ERR_INVALID and "hap_ref_pos" in capi.last_error()
    assert call(hpos=None) == capi.DD_ERR_INVALID
    assert call(out=None) == capi.DD_ERR_INVALID
    assert lib.dd_cigars_device(C.byref(db), 8, None, 8, None, C.byref(capi.dd_cigar_result(8, 8, 0, 8)), 8, None) == capi.DD_ERR_INVALID
    assert call() == capi.DD_ERR_INVALID and "offset array" in capi.last_error()   # the batch's index arrays are missing


def test_cigar_string_helper():
    ops = np.array([(3 << 4) | 4, (40 << 4) | 0, (2 << 4) | 1, (57 << 4) | 0, 0, 0], np.uint32)
    assert capi.cigar_ops(ops, 4) == [(4, 3), (0, 40), (1, 2), (0, 57)]
    assert capi.cigar_string(ops, 4) == "3S40M2I57M"
    assert capi.cigar_string(np.array([(7 << 4) | 2], np.uint32), 1) == "7D"
    try:
        capi.cigar_string(ops[:2], 4)
        assert False
    except ValueError:
        pass


def test_adversarial_set_reaches_every_branch_of_the_host_walk():
    """Before any GPU run: the generated alignments make dindel::getCIGAR take every branch, the fall-through and every throw it can reach
    (see _cigar_cases.BRANCHES for the one it cannot), with events on read bases 63, 64 and 65."""
    pb, hpos, hap_ref_pos = cc.adversarial_batch()
    took = cc.coverage(pb, hpos, hap_ref_pos)
    assert took == cc.BRANCHES, cc.BRANCHES - took
    _want, outcomes = cc.expected(pb, hpos, hap_ref_pos, None, None, 8, 0)
    codes = {o for o in outcomes if isinstance(o, int)}
    assert codes == {-4, -5, -6, -7}                                           # Error(2)!, Error(3)!, Error(4)!, How is this possible? (1)
    assert any(not isinstance(o, int) and o[1] == -1 for o in outcomes)        # whole-read clip
    assert {len(hpos[sl]) for _p, _g, sl in cc.pair_hpos_slices(pb)} >= {1, 63, 64, 65, 66, 129}
    # an event exactly on bases 63 / 64 / 65: some read has a code there while its neighbours have positions
    codes_ref = capi.hpos_reference_codes(hpos)
    at = set()
    for _p, _g, sl in cc.pair_hpos_slices(pb):
        v = codes_ref[sl]
        at |= {b for b in (63, 64, 65) if len(v) > b + 1 and v[b] < 0 <= v[b - 1]}
    assert at == {63, 64, 65}


def test_driver_help_lists_the_flag():
    exe = os.path.join(ROOT, "dindel_tgi_amd", "host", "dindel_gpu")
    text = subprocess.check_output([exe, "--help"]).decode()
    assert "--deviceCigars" in text and "--cigarOpsCap" in text and "--outputRealignedBAM" in text
