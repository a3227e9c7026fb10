"""CPU-side checks of the device realign (dd_realign_result, dd_realign_device, dd_compute_likelihoods_realign, dindel_gpu --deviceRealign):
declarations, layout, validation, no CPU fallback, the driver's flag and its refusals, and the host consumer of the realigned reads
(pooledRealignedCigars on views with hasDeviceRealign()) on hand-made views — through a C hook, and in a stand-alone program under
AddressSanitizer and UBSan.  No compute here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from dindel_tgi_amd import capi
from dindel_tgi_amd.batch import alloc_result
from tests import _cigar_cases as cc
from tests import _host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dindel_tgi_amd", "host")
M, I, D, S = 0, 1, 2, 4


def test_header_compiles_as_c99_and_layout_agrees_with_ctypes(lib, tmp_path):
    src = tmp_path / "use_realign.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dindel_hmm.h"\n'
                   'int main(void) {\n'
                   '  dd_realign_result c; (void)c;\n'
                   '  printf("%d %d %d %d %d %d\\n", (int)sizeof(dd_realign_result), (int)offsetof(dd_realign_result, hap), (int)offsetof(dd_realign_result, status),\n'
                   '         (int)offsetof(dd_realign_result, n_ops), (int)offsetof(dd_realign_result, ops), (int)offsetof(dd_realign_result, ref_off));\n'
                   '  printf("%d %d %d %d %d\\n", DD_REALIGN_OFF_HAP, DD_REALIGN_BAD_PAIR, DD_REALIGN_NO_HAPS, DD_REALIGN_FIRST_MAX, DD_REALIGN_PAIR);\n'
                   '  return dd_realign_device(NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 8, NULL) == DD_ERR_INVALID &&\n'
                   '         dd_compute_likelihoods_realign(NULL, NULL, NULL, 0, NULL, NULL, NULL, NULL, NULL, 8, 0, 0) == DD_ERR_INVALID ? 0 : 1;\n}\n')
    exe = tmp_path / "use_realign"
    libdir = os.path.join(ROOT, "dindel_tgi_amd", "csrc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", libdir, "-ldindel_hmm", "-Wl,-rpath," + libdir, "-o", str(exe)])
    import torch
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    lines = subprocess.check_output([str(exe)], env=env).decode().splitlines()
    T = capi.dd_realign_result
    assert [int(v) for v in lines[0].split()] == [C.sizeof(T), T.hap.offset, T.status.offset, T.n_ops.offset, T.ops.offset, T.ref_off.offset]
    assert [int(v) for v in lines[1].split()] == [capi.DD_REALIGN_OFF_HAP, capi.DD_REALIGN_BAD_PAIR, capi.DD_REALIGN_NO_HAPS,
                                                  capi.DD_REALIGN_FIRST_MAX, capi.DD_REALIGN_PAIR]
    assert capi.DD_REALIGN_OFF_HAP == capi.DD_CIGAR_NOT_COMPUTED + 1            # the codes continue the DD_CIGAR_* of the chosen pair
    assert lib.dd_abi_version() == capi.ABI_VERSION                            # new symbols only: the version is the parent's


def test_symbols_exist_and_the_helper_allocates_per_read(lib):
    assert hasattr(lib, "dd_realign_device") and hasattr(lib, "dd_compute_likelihoods_realign")
    assert "dd_realign_device" in capi.EXPORTS and "dd_compute_likelihoods_realign" in capi.EXPORTS
    arrs, res = capi.realign_arrays(7, 3)
    assert {k: v.shape for k, v in arrs.items()} == dict(hap=(7,), status=(7,), n_ops=(7,), ref_off=(7,), ops=(7, 3))
    assert res.ops == arrs["ops"].ctypes.data and res.hap == arrs["hap"].ctypes.data and arrs["ops"].dtype == np.uint32
    arrs0, res0 = capi.realign_arrays(0, 1)                                     # an empty batch still has addresses to hand over
    assert len(arrs0["hap"]) == 0 and res0.hap and res0.ops


def _host_call(lib, pb, mode=capi.DD_REALIGN_FIRST_MAX, ops_cap=8, hap_ref_pos="identity", pairs=None, n_indels=None, options=0, with_hpos=True,
               out="all"):
    p = capi.params_cli_defaults()
    arrs, res = alloc_result(pb)
    if not with_hpos:
        res.hpos = None
    got, rl = capi.realign_arrays(pb.n_reads, max(ops_cap, 1))
    if out is None:
        rl = None
    elif out != "all":
        setattr(rl, out, None)
    hrp = np.arange(int(pb.a["hap_seq_off"][-1]), dtype=np.int32) if isinstance(hap_ref_pos, str) else hap_ref_pos
    b = pb.ctypes_batch()
    rc = lib.dd_compute_likelihoods_realign(C.byref(p), C.byref(b), C.byref(res), mode, None if pairs is None else pairs.ctypes.data_as(capi.c_i32p),
                                            None if n_indels is None else n_indels.ctypes.data_as(capi.c_i32p),
                                            None if hrp is None else hrp.ctypes.data_as(capi.c_i32p), None, None if rl is None else C.byref(rl),
                                            ops_cap, 0, options)
    return rc, got


def test_host_entry_validates_and_has_no_cpu_fallback(lib):
    import torch
    pb = cc.csr_batch([([30], [20, 20])])
    pairs, n_indels = np.zeros(2, np.int32), np.zeros(1, np.int32)
    rc, _ = _host_call(lib, pb, ops_cap=0)
    assert rc == capi.DD_ERR_INVALID and "ops_cap" in capi.last_error()
    rc, _ = _host_call(lib, pb, hap_ref_pos=None)
    assert rc == capi.DD_ERR_INVALID and "hap_ref_pos" in capi.last_error()
    for mode in (2, -1):
        rc, _ = _host_call(lib, pb, mode=mode, pairs=pairs, n_indels=n_indels)
        assert rc == capi.DD_ERR_INVALID and "mode" in capi.last_error()
    rc, _ = _host_call(lib, pb, mode=capi.DD_REALIGN_PAIR, n_indels=n_indels)
    assert rc == capi.DD_ERR_INVALID and "win_hap_pair" in capi.last_error()
    rc, _ = _host_call(lib, pb, mode=capi.DD_REALIGN_PAIR, pairs=pairs)
    assert rc == capi.DD_ERR_INVALID and "hap_n_indels" in capi.last_error()
    for out in (None, "hap", "status", "n_ops", "ops", "ref_off"):
        rc, _ = _host_call(lib, pb, out=out)
        assert rc == capi.DD_ERR_INVALID and "dd_realign_result" in capi.last_error()
    rc, _ = _host_call(lib, pb, options=capi.DD_OPT_LONG_WINDOWS_FASTER)      # the main model's entry: only its own option bit
    assert rc == capi.DD_ERR_INVALID
    if not torch.cuda.is_available():
        for kw in (dict(), dict(with_hpos=False), dict(options=capi.DD_OPT_LONG_WINDOWS), dict(mode=capi.DD_REALIGN_PAIR, pairs=pairs, n_indels=n_indels)):
            rc, _ = _host_call(lib, pb, **kw)                                  # r->hpos == NULL is accepted: the error is the missing device
            assert rc == capi.DD_ERR_NO_DEVICE and "no CPU fallback" in capi.last_error()


def test_host_entry_marks_the_reads_of_a_batch_without_haplotypes(lib):
    """No pair, nothing to launch: every read comes back DD_REALIGN_NO_HAPS, with or without a device."""
    pb = cc.csr_batch([([], [20, 20]), ([], [7])])
    rc, got = _host_call(lib, pb)
    assert rc == 0, capi.last_error()
    assert (got["status"] == capi.DD_REALIGN_NO_HAPS).all() and (got["hap"] == -1).all() and (got["n_ops"] == 0).all() and (got["ref_off"] == -1).all()


def test_device_entry_validates_its_arguments(lib):
    db = capi.dd_device_batch()
    db.n_windows = db.n_haps = db.n_reads = 1
    out = capi.dd_realign_result(8, 8, 8, 8, 8)                                # never dereferenced: every call below is refused first
    ok = dict(mode=capi.DD_REALIGN_FIRST_MAX, ll=8, on_hap=None, pairs=None, n_indels=None, hpos=8, status=None, hrp=8, hal=None, out=C.byref(out), cap=8)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.dd_realign_device(C.byref(db), a["mode"], a["ll"], a["on_hap"], a["pairs"], a["n_indels"], a["hpos"], a["status"], a["hrp"], a["hal"],
                                     a["out"], a["cap"], None)
    assert call(cap=0) == capi.DD_ERR_INVALID and "ops_cap" in capi.last_error()
    assert call(hrp=None) == capi.DD_ERR_INVALID and "hap_ref_pos" in capi.last_error()
    assert call(hpos=None) == capi.DD_ERR_INVALID
    assert call(ll=None) == capi.DD_ERR_INVALID
    assert call(out=None) == capi.DD_ERR_INVALID
    assert call(mode=2) == capi.DD_ERR_INVALID and "mode" in capi.last_error()
    assert call(mode=capi.DD_REALIGN_PAIR, n_indels=8) == capi.DD_ERR_INVALID and "win_hap_pair" in capi.last_error()
    assert call(mode=capi.DD_REALIGN_PAIR, pairs=8) == capi.DD_ERR_INVALID and "hap_n_indels" in capi.last_error()
    for k in range(5):
        bad = [8] * 5
        bad[k] = 0
        assert call(out=C.byref(capi.dd_realign_result(*bad))) == capi.DD_ERR_INVALID and "dd_realign_result" in capi.last_error()
    assert call() == capi.DD_ERR_INVALID and "offset array" in capi.last_error()   # the batch's index arrays are missing
    assert lib.dd_realign_device(None, 0, 8, None, None, None, 8, None, 8, None, C.byref(out), 8, None) == capi.DD_ERR_INVALID


# ---------------------------------------------------------------- the driver's flag
def test_driver_help_lists_the_flag_and_refuses_the_diploid_step():
    exe = os.path.join(HOST, "dindel_gpu")
    text = subprocess.check_output([exe, "--help"]).decode()
    assert "--deviceRealign" in text and "--cigarOpsCap" in text
    for other in ("--doDiploid", "--faster"):
        r = subprocess.run([exe, "--deviceRealign", other, "--doPooled", "--outputRealignedBAM", "--bamFile", "x.bam", "--varFile", "w.txt", "--hapFile", "h.txt",
                            "--outputFile", "o"], capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout == ""
        lines = r.stderr.splitlines()
        assert len(lines) == 1 and "--deviceRealign" in lines[0] and other in lines[0]
    r = subprocess.run([exe, "--deviceRealign", "--doDiploid"], capture_output=True, text=True)        # said before anything else is asked for
    assert r.returncode != 0 and len(r.stderr.splitlines()) == 1 and "--deviceRealign" in r.stderr
    r = subprocess.run([exe, "--deviceRealign", "--outputRealignedBAM", "--bamFile", "x.bam", "--varFile", "w.txt", "--hapFile", "h.txt", "--outputFile", "o"],
                       capture_output=True, text=True)                                                  # without --doPooled the diploid step is implied
    assert r.returncode != 0 and len(r.stderr.splitlines()) == 1 and "--doPooled" in r.stderr


# ---------------------------------------------------------------- the consumer of the views, on hand-made ones
def _hook():
    lib = _host.load()
    f = lib.ddh_pooled_device_realigned_cigars
    f.argtypes = [C.c_int] * 5 + [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.POINTER(C.c_long), C.c_char_p, C.c_int]
    f.restype = C.c_int
    return f


def _consume(rows, H=3, read_len=12, hap_len=40, ops_cap=2, hpos=None, ref_seq_pos=1000, max_ops=4):
    """rows: per read (hap, status, [BAM words], ref_off, n_ops or None = len(words)) -> (rc, n_ops, ref_pos, ops, fallbacks, message)."""
    R = len(rows)
    hap = np.array([r[0] for r in rows], np.int32)
    status = np.array([r[1] for r in rows], np.int32)
    ops = np.zeros((R, ops_cap), np.uint32)
    for i, r in enumerate(rows):
        ops[i, :min(len(r[2]), ops_cap)] = r[2][:ops_cap]
    ref_off = np.array([r[3] for r in rows], np.int32)
    n_ops = np.array([len(r[2]) if len(r) < 5 else r[4] for r in rows], np.int32)
    out_n, out_pos, out_ops = np.full(R, -7, np.int32), np.full(R, -7, np.int32), np.full((R, max_ops), 0xFFFFFFFF, np.uint32)
    fb, err = C.c_long(-1), C.create_string_buffer(200)
    hp = None if hpos is None else np.ascontiguousarray(hpos, np.int16)
    assert hp is None or hp.shape == (H, R, read_len)
    rc = _hook()(H, R, read_len, hap_len, ops_cap, hap.ctypes.data, status.ctypes.data, n_ops.ctypes.data, ops.ctypes.data, ref_off.ctypes.data,
                 None if hp is None else hp.ctypes.data, ref_seq_pos, out_n.ctypes.data, out_pos.ctypes.data, out_ops.ctypes.data, max_ops, C.byref(fb), err, 200)
    return rc, out_n, out_pos, out_ops, fb.value, err.value.decode()


def w(op, ln):
    return (ln << 4) | op


def test_consumer_takes_rows_as_they_are_and_leaves_off_haplotype_reads_empty():
    rows = [(1, capi.DD_CIGAR_OK, [w(M, 12)], 13), (-1, capi.DD_REALIGN_OFF_HAP, [], -1), (2, capi.DD_CIGAR_OK, [w(S, 2), w(M, 10)], 21),
            (0, capi.DD_CIGAR_OK, [w(S, 12)], -1), (-1, capi.DD_REALIGN_NO_HAPS, [], -1)]
    rc, n, pos, ops, fb, msg = _consume(rows)
    assert rc == 0 and fb == 0, msg
    assert list(n) == [1, 0, 2, 1, 0] and list(pos) == [1013, -1, 1021, -1, -1]      # refPos = refSeqPos + ref_off; -1 stays -1
    assert list(ops[0]) == [w(M, 12), 0, 0, 0] and list(ops[2]) == [w(S, 2), w(M, 10), 0, 0] and not ops[1].any() and not ops[4].any()


@pytest.mark.parametrize("code", sorted(capi.CIGAR_MESSAGES))
def test_consumer_raises_the_string_of_every_throw_code(code):
    rows = [(0, capi.DD_CIGAR_OK, [w(M, 12)], 0), (-1, capi.DD_REALIGN_OFF_HAP, [], -1), (1, code, [], -1), (0, capi.DD_CIGAR_ERROR4 if code != capi.DD_CIGAR_ERROR4 else capi.DD_CIGAR_ERROR1, [], -1)]
    rc, _n, _pos, _ops, _fb, msg = _consume(rows)
    assert rc == -1 and msg == capi.CIGAR_MESSAGES[code]                           # reads in order: the first read that throws


def test_consumer_redoes_reads_over_the_cap_on_the_host():
    """DD_CIGAR_OVERFLOW and DD_CIGAR_NOT_COMPUTED: getCIGAR for haplotype realignHap(r) from the alignments at hand, counted; without them
    the overload says so."""
    H, R, L = 3, 4, 12
    hpos = np.zeros((H, R, L), np.int16)
    for h in range(H):
        for r in range(R):
            v = np.arange(L) + h + r
            v[L // 2:] += 2                                                         # two haplotype bases deleted: 6M2D6M on the identity map
            hpos[h, r] = v
    rows = [(2, capi.DD_CIGAR_OVERFLOW, [w(M, 6), w(D, 2)], 20, 3), (0, capi.DD_CIGAR_OK, [w(M, 12)], 1), (1, capi.DD_CIGAR_NOT_COMPUTED, [], -1, 0),
            (-1, capi.DD_REALIGN_OFF_HAP, [], -1)]
    rc, n, pos, ops, fb, msg = _consume(rows, H=H, read_len=L, hpos=hpos)
    assert rc == 0 and fb == 2, msg
    assert list(n) == [3, 1, 3, 0]
    assert list(ops[0]) == [w(M, 6), w(D, 2), w(M, 6), 0] and list(ops[2]) == list(ops[0])
    assert list(pos) == [1000 + 20 + 2 + 0, 1001, 1000 + 10 + 1 + 2, -1]               # haplotype h lies at 10 h; the read starts at base h + r
    host = cc.host_cigar(np.arange(40) + 20, hpos[2, 0])                            # the same through ddh_get_cigar
    assert host == ([(M, 6), (D, 2), (M, 6)], 22)
    rc, _n, _pos, _ops, _fb, msg = _consume(rows, H=H, read_len=L, hpos=None)
    assert rc == -1 and "no alignments are at hand" in msg
    rc, n, _pos, _ops, fb, msg = _consume(rows[1:2] + rows[3:], H=H, read_len=L, hpos=None)   # nothing over the cap: nothing is asked for
    assert rc == 0 and fb == 0 and list(n) == [1, 0]


def test_consumer_refuses_a_row_without_a_haplotype():
    for row in [(3, capi.DD_CIGAR_OK, [w(M, 12)], 0), (-1, capi.DD_CIGAR_OK, [w(M, 12)], 0), (-1, capi.DD_REALIGN_BAD_PAIR, [], -1)]:
        rc, _n, _pos, _ops, _fb, msg = _consume([(0, capi.DD_CIGAR_OK, [w(M, 12)], 0), row])
        assert rc == -1 and "no haplotype was chosen" in msg


# ---------------------------------------------------------------- the stand-alone program under the sanitizers
def test_check_program_under_address_and_undefined_sanitizers(tmp_path):
    """tests/realign_check.cpp with the adapter, the consumer and the units they stand on, g++ alone (the C ABI is stubbed in the program),
    under AddressSanitizer and UBSan; run directly."""
    exe = str(tmp_path / "realign_check")
    units = ["compute_likelihoods", "realigned_bam", "cigar", "genotype", "diploid_glf", "bam_reader", "fast_inflate"]
    subprocess.check_call(["g++", "-std=c++11", "-O0", "-g", "-pthread", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "realign_check.cpp")] + [os.path.join(HOST, u + ".cpp") for u in units] + ["-lz"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.endswith("realign_check: ok\n") and r.stderr == "", (r.stdout[-2000:], r.stderr[-4000:])
