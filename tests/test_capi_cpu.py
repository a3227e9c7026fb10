"""CPU-side checks of the C ABI: the library loads, exports every symbol include/dindel_hmm.h declares,
its host bookkeeping agrees with the numpy packer, and compute entry points refuse to run without a GPU
(there is no CPU fallback).  No compute calls here."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from dindel_tgi_amd import capi, synth
from dindel_tgi_amd.batch import ReadRec, Window, alloc_result, pack, phred_to_prob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    src = open(os.path.join(ROOT, "include", "dindel_hmm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dd_[a-z_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported(lib):
    names = declared_functions()
    assert set(names) == set(capi.EXPORTS), (names, capi.EXPORTS)
    for n in names:
        assert getattr(lib, n) is not None
    assert lib.dd_abi_version() == capi.ABI_VERSION
    assert lib.dd_kernel_name().decode() == "dd_hmm_kernel"


def test_param_defaults_match_reference_sets(lib):
    p = capi.dd_params()
    lib.dd_params_cli_defaults(C.byref(p))
    assert p.as_dict() == capi.params_cli_defaults().as_dict()
    # DInDel.cpp:4154-4157, :4122: pError 5e-4, pMut 1e-5, maxLengthIndel 5, flankRefSeq 2
    assert (p.pError, p.pMut, p.maxLengthDel, p.padCover, p.mapQualThreshold) == (5e-4, 1e-5, 5, 2, 100.0)
    lib.dd_params_struct_defaults(C.byref(p))
    assert p.as_dict() == capi.params_struct_defaults().as_dict()
    # ObservationModel.hpp:39-64
    assert (p.pError, p.pMut, p.maxLengthDel, p.padCover, p.pFirstgLO, p.checkBaseQualThreshold, p.bMid) == \
        (1e-4, 1e-4, 10, 5, 0.01, 0.95, -1)


def test_sizes_and_offsets_agree_with_packer(lib):
    pb = synth.generate(7, H=3, R=11, L=40, hap_len=50, seed=5, vary_read_len=True, mixed_quals=True)
    b = pb.ctypes_batch()
    sz = capi.dd_sizes()
    assert lib.dd_batch_sizes(C.byref(b), C.byref(sz)) == 0
    assert (sz.n_haps, sz.n_reads, sz.n_pairs) == (pb.n_haps, pb.n_reads, pb.n_pairs)
    assert (sz.hpos_len, sz.var_cov_len, sz.cells) == (pb.hpos_len, pb.var_cov_len, pb.cells)
    assert (sz.max_hap_len, sz.max_read_len) == (pb.max_hap_len, pb.max_read_len)
    po = np.zeros(pb.n_windows + 1, np.int64); ho = np.zeros_like(po); vo = np.zeros_like(po)
    hw = np.zeros(pb.n_haps, np.int32)
    assert lib.dd_build_index(C.byref(b), hw.ctypes.data_as(capi.c_i32p), po.ctypes.data_as(capi.c_i64p),
                              ho.ctypes.data_as(capi.c_i64p), vo.ctypes.data_as(capi.c_i64p)) == 0
    assert np.array_equal(po, pb.win_pair_off) and np.array_equal(ho, pb.win_hpos_off)
    assert np.array_equal(vo, pb.win_varcov_off)
    assert np.array_equal(hw, np.repeat(np.arange(pb.n_windows), np.diff(pb.a["win_hap_off"])))


def test_tables_are_the_reference_formulas(lib):
    """dd_build_tables vs the formulas of ObservationModelFB.cpp:226-234, 268-303, 1643-1703 (python math =
    the same libm)."""
    p = capi.params_cli_defaults()
    quals = phred_to_prob([2, 10, 20, 30, 41])
    mapqs = phred_to_prob([0, 20, 40, 60, 150])
    out = np.zeros(capi.DD_TABLE_DOUBLES)
    n = lib.dd_build_tables(C.byref(p), quals.ctypes.data_as(capi.c_f64p), len(quals),
                            mapqs.ctypes.data_as(capi.c_f64p), len(mapqs), out.ctypes.data_as(capi.c_f64p))
    assert 0 < n <= capi.DD_TABLE_DOUBLES
    assert out[0] == math.log(1.0 - 0.01) and out[1] == math.log(0.01) and out[2] == -0.5
    assert out[3] == math.log(1.0 - math.exp(-0.5)) and out[4] == math.log(5e-4) and out[5] == math.log(1 - 5e-4)
    TQ, TM, TH = 32, 32 + 1024, 32 + 2048
    for i, q in enumerate(quals):
        pr = q * (1.0 - p.pMut)
        assert out[TQ + 4 * i] == math.log(.25 + .75 * pr)
        assert out[TQ + 4 * i + 1] == math.log(.75 + 1e-10 - .75 * pr)
        assert out[TQ + 4 * i + 2] == math.log10(1.0 - q)
    lIns = [math.log(1.0 - math.exp(math.log(p.pError))), math.log(p.pError)]
    for i, mqv in enumerate(mapqs):
        mq = 1.0 - mqv
        if -10.0 * math.log10(mq) > p.mapQualThreshold:
            mq = math.pow(10.0, -p.mapQualThreshold / 10.0)
        for k in range(2):
            assert out[TM + 4 * i + k] == math.log(mq) + lIns[k] + 0.0
            assert out[TM + 4 * i + 2 + k] == 0.0 + math.log(1.0 - mq) + lIns[k]
    base = [2.9e-5] * 4 + [4.3e-5, 1.1e-4, 2.4e-4, 5.7e-4, 1.0e-3, 1.4e-3]
    for ln in (1, 4, 5, 10, 11, 30, 52, 63):
        pbe = (base[ln - 1] if ln <= 10 else base[9] + 4.3e-4 * float(ln - 10)) * float(ln)
        pbe = min(pbe, 0.99)
        assert out[TH + 2 * ln] == math.log(pbe) and out[TH + 2 * ln + 1] == math.log(1.0 - pbe)


def _one_window(hap="ACGTACGTACGT", read="ACGTAC"):
    return pack([Window(1000, [hap], [ReadRec(read, [0.999] * len(read), 0.9999, 1000)])])


def test_no_cpu_fallback_and_validation(lib):
    import torch
    p = capi.params_cli_defaults()
    pb = _one_window()
    arrs, res = alloc_result(pb)
    b = pb.ctypes_batch()
    if not torch.cuda.is_available():
        assert lib.dd_compute_likelihoods(C.byref(p), C.byref(b), C.byref(res), 0) == capi.DD_ERR_NO_DEVICE
        assert "no CPU fallback" in capi.last_error()
    # validation happens before any device work
    p2 = capi.params_cli_defaults(); p2.mapUnmappedReads = 1                 # needs the mate / library arrays
    assert lib.dd_compute_likelihoods(C.byref(p2), C.byref(b), C.byref(res), 0) == capi.DD_ERR_INVALID
    assert "mapUnmappedReads" in capi.last_error()
    p4 = capi.params_cli_defaults(); p4.forceReadOnHaplotype = 1
    assert lib.dd_compute_likelihoods(C.byref(p4), C.byref(b), C.byref(res), 0) == capi.DD_ERR_UNSUPPORTED
    p3 = capi.params_cli_defaults(); p3.maxLengthDel = 32                   # 0..31 are supported (12..31 on the one D = 32 build)
    assert lib.dd_compute_likelihoods(C.byref(p3), C.byref(b), C.byref(res), 0) == capi.DD_ERR_UNSUPPORTED and "[0,31]" in capi.last_error()
    res2 = capi.dd_result()
    assert lib.dd_compute_likelihoods(C.byref(p), C.byref(b), C.byref(res2), 0) == capi.DD_ERR_INVALID


def test_missing_extension_fails_loudly(monkeypatch):
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi, "LIB_PATH", "/nonexistent/libdindel_hmm.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        capi.load()


def test_symbol_lut(lib):
    """dd_build_symbol_lut: A,C,G,T,N fixed; other haplotype bytes get ids 5..30 in byte order; all remaining bytes 31."""
    pb = pack([Window(1000, ["ACGTNRYacgtn", "MMKA"], [ReadRec("ACGTWS", [0.999] * 6, 0.9999, 1000)])])
    b = pb.ctypes_batch()
    lut = np.zeros(256, np.uint8)
    assert lib.dd_build_symbol_lut(C.byref(b), lut.ctypes.data_as(C.POINTER(C.c_uint8))) == 0
    assert [int(lut[ord(c)]) for c in "ACGTN"] == [0, 1, 2, 3, 4]
    others = sorted(set("RYacgtnMK"))
    assert [int(lut[ord(c)]) for c in others] == list(range(5, 5 + len(others)))
    assert int(lut[ord("W")]) == 31 and int(lut[ord("S")]) == 31 and int(lut[0]) == 31


def test_header_is_plain_c_and_links(tmp_path):
    """include/dindel_hmm.h must be usable from C (the reference-side binding is cgo/JNI/ctypes-like): compile a C99
    translation unit against it, link the shared library, and call the housekeeping entry points."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "use_abi.c"
    src.write_text('#include <stdio.h>\n#include "dindel_hmm.h"\n'
                   'int main(void) {\n'
                   '  dd_params p; dd_batch b; dd_result r; dd_device_batch db; dd_sizes sz;\n'
                   '  dd_params_cli_defaults(&p);\n'
                   '  (void)b; (void)r; (void)db; (void)sz;\n'
                   '  printf("%d %d %g %d\\n", dd_abi_version(), DD_ABI_VERSION, p.pError, (int)sizeof(dd_batch));\n'
                   '  return dd_abi_version() == DD_ABI_VERSION ? 0 : 1;\n}\n')
    exe = tmp_path / "use_abi"
    libdir = os.path.join(root, "dindel_tgi_amd", "csrc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(root, "include"), str(src),
                           "-L", libdir, "-ldindel_hmm", "-Wl,-rpath," + libdir, "-o", str(exe)])
    import torch
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.check_output([str(exe)], env=env).decode().split()
    assert out[0] == out[1] and float(out[2]) == 5e-4
    # the ctypes mirror has the same struct size as the C compiler sees
    assert int(out[3]) == C.sizeof(capi.dd_batch)


def test_launch_plan_rules(lib, monkeypatch):
    """dd_plan_info (no device needed) pins the launch heuristics the GPU sweeps settled (profiles/r01/plan_check.jsonl,
    coverage_sweep.jsonl, batch_size_sweep.jsonl)."""
    def plan(mld=5, hap=120, L=100, reads=200, haps=80000):
        p = capi.params_cli_defaults(); p.maxLengthDel = mld
        out = (C.c_int32 * 10)()
        assert lib.dd_plan_info(C.byref(p), hap, L, 1, reads, haps, C.byref(out)) == 0, capi.last_error()
        return dict(K=out[0], D=out[1], hbm=out[2], waves=out[3], split=out[4], lds=out[5], scratch_kib=out[6], waves_cu=out[7], G=out[8])
    # lane tiling by haplotype length: numS = Hs+2 <= 64 K on a whole wavefront, or <= 32 K on a half (two pairs per wavefront, round 4)
    # where that is the tighter fit and measured faster: <= 30, 63..94, 127..158 bp
    hs = (30, 31, 62, 63, 94, 95, 126, 127, 158, 159, 190, 191, 222, 223, 254, 255, 318, 319, 382, 383, 446, 447, 510, 511, 702, 703, 766)
    assert [(plan(hap=h)["G"], plan(hap=h)["K"]) for h in hs] == \
        [(2, 1), (1, 1), (1, 1), (2, 3), (2, 3), (1, 2), (1, 2), (2, 5), (2, 5), (1, 3), (1, 3), (1, 4), (1, 4), (1, 4), (1, 4), (1, 5), (1, 5),
         (1, 6), (1, 6), (1, 7), (1, 7), (1, 8), (1, 8), (1, 9), (1, 11), (1, 12), (1, 12)]
    monkeypatch.setenv("DD_NO_HALF", "1")                      # A/B switch: whole-wavefront tilings only
    assert [(plan(hap=h)["G"], plan(hap=h)["K"]) for h in (30, 62, 63, 127, 191, 222)] == [(1, 1), (1, 1), (1, 2), (1, 3), (1, 4), (1, 4)]
    monkeypatch.delenv("DD_NO_HALF")
    assert [(plan(hap=h, mld=10)["G"], plan(hap=h, mld=10)["K"]) for h in (30, 94, 158, 222)] == [(2, 1), (2, 3), (2, 5), (1, 4)]   # the same tilings on the D = 11 build
    # D routing: a smaller D runs on the next larger specialised build
    assert [plan(mld=m)["D"] for m in range(12)] == [6] * 6 + [11] * 5 + [12]
    # maxLengthDel 12..31 (the reference takes any --maxLengthIndel, DInDel.cpp:4157): one D = 32 build, whole wavefronts, scratch back-pointers, up to 574 bp
    assert [(plan(mld=m, hap=h)["D"], plan(mld=m, hap=h)["G"], plan(mld=m, hap=h)["hbm"]) for m, h in ((12, 140), (20, 80), (31, 574))] == [(32, 1, 1)] * 3
    out = (C.c_int32 * 10)()
    p32 = capi.params_cli_defaults(); p32.maxLengthDel = 12
    assert lib.dd_plan_info(C.byref(p32), 575, 100, 1, 200, 8, C.byref(out)) == capi.DD_ERR_UNSUPPORTED and "574" in capi.last_error()
    # LDS tile while it costs no resident wave, HBM scratch beyond (K=2: reads up to ~115 bp), and always for K >= 4 / K = 3 at D > 6
    assert [plan(L=l)["hbm"] for l in (36, 100, 110, 120, 150, 250, 1000)] == [0, 0, 0, 1, 1, 1, 1]
    assert plan(hap=170)["hbm"] == 1 and plan(hap=170)["scratch_kib"] > 0 and plan()["scratch_kib"] == 0
    # end of round 4 (the item counter made the scratch builds 10-18 % faster): scratch for every K >= 3 whatever the read length, and for K = 2
    # above D = 7 (profiles/r04/plan_check.jsonl; before: K = 3 / D = 6 on the LDS tile up to 90-bp reads, K = 4 / D = 6 up to 80 bp, K = 2 / D = 11 up to ~100)
    assert [plan(hap=170, L=l)["hbm"] for l in (36, 76, 90, 100, 150)] == [1] * 5
    assert plan(hap=170, L=76, mld=10)["hbm"] == 1 and plan(hap=200, L=100)["hbm"] == 1
    assert [plan(hap=240, L=l)["hbm"] for l in (36, 76, 80, 81, 100)] == [1] * 5 and plan(hap=240, L=76, mld=10)["hbm"] == 1
    assert [plan(mld=10, L=l)["hbm"] for l in (36, 76, 100)] == [1] * 3 and plan(mld=10, hap=43, L=76)["hbm"] == 0      # (K = 1 keeps the LDS rule)
    assert plan()["waves"] == 4 and plan()["waves_cu"] == 12 and plan()["lds"] <= 160 * 1024
    # workgroup size follows how well the windows' reads fill the waves
    assert [plan(reads=r)["waves"] for r in (1, 2, 3, 5, 10, 20, 200)] == [1, 2, 3, 1, 2, 4, 4]
    # read split: none for big batches; small batches split down to one round of reads per wave
    # (round 3: the split also weighs how the grid fills the 768 workgroups the chip holds at once, profiles/r03/split_ab.txt)
    assert plan(haps=80000)["split"] == 1 and plan(haps=8)["split"] == 50 and plan(haps=512)["split"] == 10
    assert plan(haps=2048)["split"] == 3 and plan(haps=4096)["split"] == 2 and plan(haps=1024)["split"] == 5
    p = capi.params_cli_defaults()
    out = (C.c_int32 * 10)()
    assert lib.dd_plan_info(C.byref(p), 767, 100, 1, 200, 8, C.byref(out)) == capi.DD_ERR_UNSUPPORTED


def test_full_length_haplotypes_leave_the_folded_launch(lib, monkeypatch):
    """The folded builds (K <= 2, D = 6) need 64 K >= Hs + 3 for every haplotype of their launch: a few haplotypes of exactly 126 (62) bp go to a launch of
    their own (same tiling, not folded) so that the thousands of shorter ones keep the fold; many of them stay where they are."""
    rng = np.random.default_rng(9)
    def batch(n_short, n_full, full=126):
        wins = []
        for i in range(n_short + n_full):
            hl = full if i >= n_short else int(rng.integers(full - 16, full))
            hap = "".join(rng.choice(list("ACGT"), hl))
            wins.append(Window(1000, [hap], [ReadRec(hap[:40], [0.99] * 40, 0.99, 1000)]))
        return pack(wins)
    def classes(pb, params=True):
        b = pb.ctypes_batch()
        cls = capi.dd_length_classes()
        lst = np.zeros(pb.n_haps * capi.N_READ_CLASSES, np.int32)
        p = capi.params_cli_defaults()
        assert lib.dd_build_length_classes(C.byref(b), None, C.byref(p) if params else None, lst.ctypes.data_as(capi.c_i32p), C.byref(cls)) == 0
        return [(cls.launch[i].hap_class, cls.launch[i].list_len, cls.launch[i].max_hap_len) for i in range(cls.n_launches)]
    pb = batch(200, 3)
    assert classes(pb) == [(3, 200, 125), (3, 3, 126)]                    # the three 126-bp haplotypes run apart
    monkeypatch.setenv("DD_NO_PROMOTE", "1")
    assert classes(pb) == [(3, 203, 126)]
    monkeypatch.delenv("DD_NO_PROMOTE")
    assert classes(batch(200, 60)) == [(3, 260, 126)]                      # too many to move (more than a quarter of the others)
    assert classes(pb, params=False) == [(3, 203, 126)]                    # no parameters, no plan: nothing moves
    p10 = capi.params_cli_defaults(); p10.maxLengthDel = 10                # the D = 11 build has no folded variant on the plan's path
    b = pb.ctypes_batch(); cls = capi.dd_length_classes(); lst = np.zeros(pb.n_haps * capi.N_READ_CLASSES, np.int32)
    assert lib.dd_build_length_classes(C.byref(b), None, C.byref(p10), lst.ctypes.data_as(capi.c_i32p), C.byref(cls)) == 0 and cls.n_launches == 1
    assert classes(batch(300, 2, full=62)) == [(1, 300, 61), (1, 2, 62)]   # K = 1 likewise


def test_length_classes_and_library_tables_on_the_host(lib):
    """dd_build_length_classes and dd_build_library_tables are pure host helpers: checked here without a device."""
    rng = np.random.default_rng(8)
    wins = []
    for hl, L in ((50, 36), (62, 100), (63, 100), (126, 161), (127, 160), (400, 300), (766, 1024)):
        hap = "".join(rng.choice(list("ACGT"), hl))
        wins.append(Window(1000, [hap, hap[:hl // 2] + hap[hl // 2 + 1:]], [ReadRec(hap[:min(L, hl)].ljust(L, "A"), [0.99] * L, 0.99, 1000)]))
    probs = np.array([0.1, 0.2, 0.3, 0.4])
    pb = pack(wins, libraries=[(probs, 0.3), (np.array([1.0]), 1.0)])
    b = pb.ctypes_batch()
    cls = capi.dd_length_classes()
    lst = np.zeros(pb.n_haps * capi.N_READ_CLASSES, np.int32)
    p = capi.params_cli_defaults()
    assert lib.dd_build_length_classes(C.byref(b), None, C.byref(p), lst.ctypes.data_as(capi.c_i32p), C.byref(cls)) == 0
    hl = np.diff(pb.a["hap_seq_off"])
    rl = np.diff(pb.a["read_seq_off"])
    hc = np.searchsorted(capi.HAP_CLASS_BOUNDS, hl, side="left")             # one class per lane tiling (plan.cpp kHapClasses)
    hw = np.repeat(np.arange(pb.n_windows), np.diff(pb.a["win_hap_off"]))
    # every window here has ONE read, so each haplotype is in exactly one launch: that of (its tiling, its read's interval)
    launches = [cls.launch[i] for i in range(cls.n_launches)]
    assert cls.list_len == pb.n_haps == sum(L.list_len for L in launches)
    seen = []
    for L in launches:
        seg = lst[L.list_off:L.list_off + L.list_len]
        assert (np.diff(seg) > 0).all() and (hc[seg] == L.hap_class).all() and L.max_hap_len == int(hl[seg].max())
        r = rl[hw[seg]]                                                      # the one read of each listed haplotype's window
        assert (r >= L.min_read_len).all() and L.max_read_len == int(r.max()) and L.max_window_reads == L.avg_window_reads == 1
        seen += seg.tolist()
    assert sorted(seen) == list(range(pb.n_haps))
    # read classes: windows whose longest read is <= T (back-pointer tile in LDS at full occupancy), the other windows' reads up to 160 bp, reads > 160 bp
    k2 = [L for L in launches if L.hap_class == 3]                           # 95..126 bp: the (126, 161) window and the shorter haplotype of (127, 160)
    assert [(L.max_read_len, L.list_len) for L in k2] == [(160, 1), (161, 2)] and k2[1].min_read_len == 161 and k2[0].min_read_len == 1
    k1 = [L for L in launches if L.hap_class == 1]                           # 31..62 bp: (50, 36), (62, 100) and the shorter haplotype of (63, 100)
    assert [(L.min_read_len, L.max_read_len, L.list_len) for L in k1] == [(1, 100, 5)]
    # without params there is no cut at T: [1, 160], (160, 1024]
    assert lib.dd_build_length_classes(C.byref(b), None, None, lst.ctypes.data_as(capi.c_i32p), C.byref(cls)) == 0
    assert sorted({cls.launch[i].min_read_len for i in range(cls.n_launches)}) == [1, 161]
    lp = np.zeros(5); l95 = np.zeros(2)
    assert lib.dd_build_library_tables(C.byref(b), lp.ctypes.data_as(capi.c_f64p), l95.ctypes.data_as(capi.c_f64p)) == 0
    assert lp.tolist() == [math.log(x) for x in (0.1, 0.2, 0.3, 0.4, 1.0)] and l95.tolist() == [math.log(0.3), 0.0]
    bad = pack(wins, libraries=[(np.array([0.5, 0.0]), 0.5)])
    assert lib.dd_build_library_tables(C.byref(bad.ctypes_batch()), lp.ctypes.data_as(capi.c_f64p), l95.ctypes.data_as(capi.c_f64p)) == capi.DD_ERR_INVALID


def test_screen_windows_flags_only_the_offending_windows(lib):
    """dd_screen_windows: a haplotype > 766 bp, a read > 1024 bp or an empty read / haplotype flags ITS window; the maxima
    are those of the windows that pass; dd_build_length_classes keeps skipped haplotypes out of the class maxima."""
    rng = np.random.default_rng(9)
    def seq(n):
        return "".join(rng.choice(list("ACGT"), n))
    good = Window(1000, [seq(100), seq(130)], [ReadRec(seq(80), [0.99] * 80, 0.99, 1000)])
    long_hap = Window(1000, [seq(767), seq(50)], [ReadRec(seq(40), [0.99] * 40, 0.99, 1000)])
    long_read = Window(1000, [seq(60)], [ReadRec(seq(1025), [0.99] * 1025, 0.99, 1000), ReadRec(seq(30), [0.99] * 30, 0.99, 1000)])
    empty_read = Window(1000, [seq(60)], [ReadRec("", [], 0.99, 1000)])
    limit = Window(1000, [seq(766)], [ReadRec(seq(1024), [0.99] * 1024, 0.99, 1000)])
    pb = pack([good, long_hap, long_read, good, empty_read])
    b = pb.ctypes_batch()
    skip = np.full(pb.n_windows, 7, np.uint8)
    mx = (C.c_int32 * 2)()
    assert lib.dd_screen_windows(C.byref(b), skip.ctypes.data_as(capi.c_u8p), C.byref(mx)) == 3
    assert skip.tolist() == [0, 1, 1, 0, 1] and list(mx) == [130, 80]
    cls = capi.dd_length_classes()
    lst = np.zeros(pb.n_haps * capi.N_READ_CLASSES, np.int32)
    p = capi.params_cli_defaults()
    assert lib.dd_build_length_classes(C.byref(b), skip.ctypes.data_as(capi.c_u8p), C.byref(p), lst.ctypes.data_as(capi.c_i32p), C.byref(cls)) == 0
    # the haplotypes of the skipped windows (2, 3, 4, 7) ride in the first launch without counting towards its maxima
    L0, L1 = cls.launch[0], cls.launch[1]
    assert cls.n_launches == 2 and cls.list_len == pb.n_haps
    assert lst[L0.list_off:L0.list_off + L0.list_len].tolist() == [0, 2, 3, 4, 5, 7] and (L0.hap_class, L0.max_hap_len, L0.max_read_len) == (3, 100, 80)
    assert lst[L1.list_off:L1.list_off + L1.list_len].tolist() == [1, 6] and (L1.hap_class, L1.max_hap_len, L1.max_read_len) == (4, 130, 80)
    assert lib.dd_build_length_classes(C.byref(b), None, C.byref(p), lst.ctypes.data_as(capi.c_i32p), C.byref(cls)) == capi.DD_ERR_UNSUPPORTED
    pb2 = pack([limit, good])
    assert lib.dd_screen_windows(C.byref(pb2.ctypes_batch()), skip.ctypes.data_as(capi.c_u8p), C.byref(mx)) == 0
    assert list(mx) == [766, 1024]


def test_screen_windows_odd_bytes_beyond_the_symbol_table(lib):
    """The main kernel's symbol table holds 26 non-ACGTN byte values per batch (in byte order).  Windows whose haplotypes use a value that
    got none are flagged one by one (round 2 failed the whole call); with 26 or fewer nothing is flagged, whatever the bytes are."""
    odd = "".join(chr(c) for c in range(97, 97 + 29) if chr(c) not in "acgtn")           # b d e f ... : 24 lower-case letters + '{' '|' '}'
    assert len(set(odd)) == 24
    rd = [ReadRec("ACGTAC", [0.999] * 6, 0.9999, 1000)]
    plain = Window(1000, ["ACGTACGTNN"], rd)
    w24 = Window(1000, ["ACGT" + odd], rd)
    low = Window(1000, ["ACGT!#"], rd)                                                     # two more, small byte values: they get ids 5, 6
    high = Window(1000, ["ACGT~"], rd)                                                     # the 27th distinct value in byte order
    both = Window(1000, ["AC~GT", "ACGT"], rd)
    skip = np.full(8, 7, np.uint8)
    mx = (C.c_int32 * 2)()
    pb = pack([plain, w24, low])                                                           # 26 distinct: everything fits
    assert lib.dd_screen_windows(C.byref(pb.ctypes_batch()), skip.ctypes.data_as(capi.c_u8p), C.byref(mx)) == 0
    pb = pack([plain, w24, low, high, plain, both])                                        # 27: only the windows holding '~' go
    assert lib.dd_screen_windows(C.byref(pb.ctypes_batch()), skip.ctypes.data_as(capi.c_u8p), C.byref(mx)) == 2
    assert skip[:6].tolist() == [0, 0, 0, 1, 0, 1] and list(mx) == [28, 6]
    lut = np.zeros(256, np.uint8)
    assert lib.dd_build_symbol_lut(C.byref(pb.ctypes_batch()), lut.ctypes.data_as(C.POINTER(C.c_uint8))) == 0
    assert int(lut[ord("!")]) == 5 and int(lut[ord("#")]) == 6 and int(lut[ord("}")]) == 30 and int(lut[ord("~")]) == 31


def test_partition_windows_balances_cells(lib):
    """dd_partition_windows (the split dd_compute_likelihoods_multi uses): contiguous, covering, and balanced by
    sum(H*R*L*Hs) — not by window count — on windows of very different weight."""
    rng = np.random.default_rng(10)
    ws = []
    for i in range(40):
        hl = int(rng.integers(20, 200)); nr = int(rng.integers(0, 12)) * (8 if i % 7 == 0 else 1)
        hap = "".join(rng.choice(list("ACGT"), hl))
        ws.append(Window(1000, [hap] * int(rng.integers(1, 4)), [ReadRec(hap[:30].ljust(30, "A"), [0.99] * 30, 0.99, 1000)] * nr))
    pb = pack(ws)
    b = pb.ctypes_batch()
    hl = np.diff(pb.a["hap_seq_off"]).astype(np.int64); rl = np.diff(pb.a["read_seq_off"]).astype(np.int64)
    cells = np.array([hl[pb.a["win_hap_off"][w]:pb.a["win_hap_off"][w + 1]].sum() * rl[pb.a["win_read_off"][w]:pb.a["win_read_off"][w + 1]].sum()
                      for w in range(pb.n_windows)], np.float64)
    assert cells.sum() == pb.cells
    for n in (1, 2, 3, 8, 64):
        bounds = np.zeros(n + 1, np.int32)
        assert lib.dd_partition_windows(C.byref(b), n, bounds.ctypes.data_as(capi.c_i32p)) == 0
        assert bounds[0] == 0 and bounds[-1] == pb.n_windows and (np.diff(bounds) >= 0).all()
        if n <= 8:
            per = np.array([cells[bounds[i]:bounds[i + 1]].sum() for i in range(n)])
            assert per.max() <= cells.sum() / n + cells.max()          # no block exceeds its share by more than one window
    empty = pack([Window(1000, ["ACGT"], [])] * 3)
    bounds = np.zeros(3, np.int32)
    assert lib.dd_partition_windows(C.byref(empty.ctypes_batch()), 2, bounds.ctypes.data_as(capi.c_i32p)) == 0
    assert bounds[0] == 0 and bounds[2] == 3
