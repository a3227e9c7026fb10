"""GPU, end to end: device CIGARs through the C++ adapter (LikelihoodEngine::setDeviceCigars, the lazy views, the realignedCigars
overload) against the host path, and through the window loop: `dindel_gpu --outputRealignedBAM --deviceCigars` writes the same files byte
for byte, brings no per-base alignment back, and redoes on the host exactly the reads whose CIGAR does not fit --cigarOpsCap."""
import ctypes as C
import glob
import json
import os
import re
import subprocess

import numpy as np
import pytest

from dindel_tgi_amd import capi
from dindel_tgi_amd.batch import ReadRec, Window
from tests import _bamwriter as bw
from tests import _cigar_cases as cc
from tests import _host
from tests.test_n2_driver_gpu import HOST, scene  # noqa: F401  (the synthetic BAM / window / haplotype files)

pytestmark = pytest.mark.gpu


def adapter_cigars(windows, params, hap_ref_pos, hap_aligned, ops_cap, device=0):
    """ddh_device_cigars_json: every haplotype pair of every window, host realignedCigars against the device-CIGAR overload."""
    lib = _host.load()
    haps = [h for w in windows for h in w.haps]
    reads = [r for w in windows for r in w.reads]
    nh = np.asarray([len(w.haps) for w in windows], np.int32)
    nr = np.asarray([len(w.reads) for w in windows], np.int32)
    q = np.ascontiguousarray(np.concatenate([np.asarray(r.qual, np.float64).reshape(-1) for r in reads] + [np.zeros(1)]))
    mq = np.asarray([r.mapQual for r in reads] + [0.0], np.float64)
    pf = np.asarray([float(r.start) for r in reads] + [0.0], np.float64)
    um = np.asarray([int(r.unmapped) for r in reads] + [0], np.int32)
    lp = np.asarray([w.hap_start & 0xFFFFFFFF for w in windows], np.uint32)
    pd, pi = _host._params(params)
    hrp = np.ascontiguousarray(hap_ref_pos, np.int32)
    hal = np.ascontiguousarray(hap_aligned, np.int32)
    assert len(hrp) == sum(len(h) for h in haps) and len(hal) == len(haps)
    out = C.create_string_buffer(1 << 16)
    n = lib.ddh_device_cigars_json(len(windows), nh.ctypes.data_as(capi.c_i32p), nr.ctypes.data_as(capi.c_i32p), "\n".join(haps).encode(),
                                   "\n".join(r.seq for r in reads).encode(), q.ctypes.data_as(capi.c_f64p), mq.ctypes.data_as(capi.c_f64p),
                                   pf.ctypes.data_as(capi.c_f64p), um.ctypes.data_as(capi.c_i32p), lp.ctypes.data_as(capi.c_u32p), pd, pi,
                                   hrp.ctypes.data_as(capi.c_i32p), hal.ctypes.data_as(capi.c_i32p), ops_cap, device, out, len(out))
    assert n > 0, n
    return json.loads(out.value.decode())


def test_adapter_lazy_views_equal_host_realigned_cigars():
    from tests.test_gpu_fuzz import make_windows
    rng = np.random.default_rng(512)
    p = capi.params_cli_defaults()
    ws = make_windows(rng, 30, 140, 150, min_hap=p.maxLengthDel)
    ws.insert(5, Window(1000, ["ACG", "ACGTACGTAC"], [ReadRec("ACGTA", [0.999] * 5, 0.9999, 1000)]))      # hapSize error.: fails alone
    haps = [h for w in ws for h in w.haps]
    hrp = np.concatenate([np.asarray(cc.hap_ref_map(rng, len(h), 0.02, 0.02), np.int32) for h in haps])
    hal = (rng.random(len(haps)) > 0.1).astype(np.int32)
    res = adapter_cigars(ws, p, hrp, hal, 8)
    assert res["mismatch"] == 0, res
    assert res["pairs"] > 40 and res["thrown"] > 0 and res["views"] >= 25
    assert res["hpos_bytes"] == 0 and res["cigar_bytes"] > 0 and res["host_hpos_bytes"] > 0
    # a cap of 2: most reads overflow and are redone with getCIGAR on the host; the outcome is the same
    tight = adapter_cigars(ws, p, hrp, hal, 2)
    assert tight["mismatch"] == 0 and tight["fallbacks"] > res["fallbacks"] and tight["fallbacks"] > 20, tight
    assert tight["hpos_bytes"] == 0


def drive(scene, prefix, *extra):
    import torch
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = str(scene["tmp"] / prefix)
    res = subprocess.run([os.path.join(HOST, "dindel_gpu"), "--bamFile", scene["bam"], "--varFile", scene["vf"], "--hapFile", scene["hf"],
                          "--outputFile", out, "--quiet", "--timing", *extra], env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    timing = [l for l in res.stdout.split("\n") if l.startswith("timing:")][0]
    fields = {k: int(v) for k, v in re.findall(r"(hpos_bytes|cigar_bytes|cigar_host_fallbacks|fallback_hpos_bytes|launches)=(\d+)", timing)}
    files = {os.path.basename(f)[len(prefix):]: open(f, "rb").read() for f in sorted(glob.glob(out + ".*"))}
    return fields, files


def test_driver_device_cigars_write_the_same_files(scene):  # noqa: F811
    base_t, base = drive(scene, "dcbase", "--outputRealignedBAM")
    assert base_t["hpos_bytes"] > 0 and base_t["cigar_bytes"] == 0 and base_t["cigar_host_fallbacks"] == 0
    assert sum(1 for k in base if k.startswith(".ra.")) == 3 and ".glf.txt" in base
    dev_t, dev = drive(scene, "dcdev", "--outputRealignedBAM", "--deviceCigars")
    assert dev == base                                                    # every realigned BAM and the .glf.txt, byte for byte
    assert dev_t["hpos_bytes"] == 0 and dev_t["cigar_bytes"] > 0
    assert dev_t["cigar_host_fallbacks"] == 0 and dev_t["fallback_hpos_bytes"] == 0
    # a small cap forces the host fallback: same files, and exactly the reads with more operations than the cap are redone
    # (every read of these windows is placed on a haplotype, so its record carries the CIGAR that was computed for it)
    tight_t, tight = drive(scene, "dctight", "--outputRealignedBAM", "--deviceCigars", "--cigarOpsCap", "2")
    assert tight == base
    want = 0
    for name, blob in base.items():
        if name.startswith(".ra."):
            _h, _r, recs = bw.read_bam(str(scene["tmp"] / ("dcbase" + name)))
            want += sum(1 for r in recs if len(bw.parse_cigar(r["cigar"])) > 2)
    assert want > 10 and tight_t["cigar_host_fallbacks"] == want, (tight_t, want)
    assert tight_t["hpos_bytes"] == 0 and tight_t["fallback_hpos_bytes"] > 0
    # the flag modifies --outputRealignedBAM only
    plain_t, plain = drive(scene, "dcplain")
    alone_t, alone = drive(scene, "dcalone", "--deviceCigars")
    assert alone == plain and alone_t["cigar_bytes"] == 0 and alone_t["hpos_bytes"] == plain_t["hpos_bytes"] == 0
