#!/usr/bin/env python3
"""Host decisions of the library as text, for comparing two builds byte for byte (no GPU needed).

    DD_LIB_PATH=<a libdindel_hmm.so> python tools/host_equivalence.py OUT.txt [--reduced]

Walks a fixed, seeded grid over everything the library decides on the host — launch plans, workspace sizes, launch classes of
ragged batches, window screens, sizes / offsets / partitions, the host tables (as raw bytes), and the refusals with their
dd_last_error() texts — and writes one record per line.  Two libraries that decide alike give identical files (`cmp`).
Prints the number of records.  --reduced: a thinner grid (seconds), what tests/test_tools_cpu.py runs."""
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from dindel_tgi_amd import capi, synth
from dindel_tgi_amd.batch import ReadRec, Window, alloc_result, pack

REDUCED = "--reduced" in sys.argv
lib = capi.load()
out = []


def rec(*parts):
    out.append(" ".join(str(p) for p in parts))


def err():
    return repr(capi.last_error())


def digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


class env:
    """One DD_* switch for the calls inside (the library reads these per call)."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k in self.kv:
            del os.environ[k]


def params(mld=None, cli=True):
    p = capi.params_cli_defaults() if cli else capi.params_struct_defaults()
    if mld is not None:
        p.maxLengthDel = mld
    return p


# ---- launch plans ----
MLD = [0, 4, 5, 9, 10, 11, 12, 20, 31]
HAPS = sorted({h for b in capi.HAP_CLASS_BOUNDS for h in (b - 1, b, b + 1) if 1 <= h <= 766} | {1})
READS = [36, 80, 100, 115, 116, 150, 160, 161, 250, 400, 1024]
AVG = [1, 2, 10, 50, 200]
NHAPS = [8, 800, 80000]
if REDUCED:
    MLD, HAPS, READS, AVG, NHAPS = [5, 10, 12], HAPS[::4], [36, 100, 160, 400], [2, 200], [8, 80000]


def plan_grid(tag):
    o = (C.c_int32 * 10)()
    for mld in MLD:
        p = params(mld)
        for hap in HAPS:
            for L in READS:
                for avg in AVG:
                    for nh in NHAPS:
                        rc = lib.dd_plan_info(C.byref(p), hap, L, 1, avg, nh, C.byref(o))
                        rec("plan", tag, mld, hap, L, avg, nh, rc, *(list(o) if rc == 0 else [err()]))


plan_grid("-")
for k, v in [("DD_NO_HALF", "1"), ("DD_FORCE_GBT", "0"), ("DD_FORCE_GBT", "1"), ("DD_REG_WAVES", "8")]:
    with env(**{k: v}):
        plan_grid("%s=%s" % (k, v))
o = (C.c_int32 * 10)()
for args in [(0, 100, 1, 10, 8), (767, 100, 1, 10, 8), (100, 0, 1, 10, 8), (100, 1025, 1, 10, 8)]:
    rec("plan-refused", args, lib.dd_plan_info(C.byref(params()), *args, C.byref(o)), err())
rec("plan-refused null-out", lib.dd_plan_info(C.byref(params()), 100, 100, 1, 10, 8, None), err())
rec("plan-refused null-params", lib.dd_plan_info(None, 100, 100, 1, 10, 8, C.byref(o)), err())

# ---- workspace sizes ----
for fn in ("dd_workspace_bytes", "dd_workspace_bytes_long", "dd_workspace_bytes_faster_long"):
    getattr(lib, fn).restype = C.c_size_t
cls = capi.dd_length_classes()
cls.n_launches = 3
for i, (mh, mr) in enumerate([(62, 100), (126, 160), (254, 400)]):
    cls.launch[i].max_hap_len, cls.launch[i].max_read_len, cls.launch[i].min_read_len = mh, mr, 1
for mld in ([5, 12] if REDUCED else MLD):
    p = params(mld)
    for W in [1, 64, 10000]:
        for hap in (HAPS[::2] if REDUCED else HAPS):
            for L in READS:
                for with_classes in (0, 1):
                    db = capi.dd_device_batch()
                    db.n_windows, db.n_haps, db.n_reads, db.max_hap_len, db.max_read_len, db.n_qual = W, 8 * W, 50 * W, hap, L, 3
                    if with_classes:
                        db.classes = C.cast(C.pointer(cls), C.c_void_p)
                        db.hap_class_list = 64            # (never followed on the host: only its presence counts)
                    rec("ws", mld, W, hap, L, with_classes, lib.dd_workspace_bytes(C.byref(p), C.byref(db)))
        for lh, lr in [(767, 100), (1000, 1025), (2048, 2048), (4094, 4096), (4095, 100), (100, 4097), (0, 0)]:
            db = capi.dd_device_batch()
            db.n_windows, db.n_haps, db.n_reads, db.n_qual, db.long_max_hap_len, db.long_max_read_len = W, 8 * W, 50 * W, 3, lh, lr
            rec("ws-long", mld, W, lh, lr, lib.dd_workspace_bytes_long(C.byref(p), C.byref(db)),
                lib.dd_workspace_bytes_faster_long(C.byref(p), C.byref(db)))

# ---- launch classes of ragged batches (what bench.py --ragged-only runs) ----
def length_classes(tag, pb, skip, p):
    b = pb.ctypes_batch()
    lc = capi.dd_length_classes()
    lst = np.full(pb.n_haps * capi.N_READ_CLASSES + 1, -1, np.int32)
    rc = lib.dd_build_length_classes(C.byref(b), skip.ctypes.data_as(capi.c_u8p) if skip is not None else None,
                                     C.byref(p) if p is not None else None, lst.ctypes.data_as(capi.c_i32p), C.byref(lc))
    rec("classes", tag, rc, err() if rc else "", digest(np.frombuffer(bytes(lc), np.uint8)) if rc == 0 else "", digest(lst))
    for i in range(lc.n_launches if rc == 0 else 0):
        rec("  launch", tag, i, *[getattr(lc.launch[i], f) for f, _ in capi.dd_launch_class._fields_])


ragged = [synth.generate_ragged(n, seed=s) for n, s in ([(40, 1)] if REDUCED else [(40, 1), (300, 0x5EED4), (1000, 7), (300, 99)])]
for i, pb in enumerate(ragged):
    skip = (np.arange(pb.n_windows) % 7 == 3).astype(np.uint8)
    for mld in (5, 10, 12):
        for sk in (None, skip):
            length_classes("r%d mld%d skip%d" % (i, mld, sk is not None), pb, sk, params(mld))
    length_classes("r%d null-params" % i, pb, None, None)
    for k, v in [("DD_NO_FOLD", "1"), ("DD_NO_PROMOTE", "1"), ("DD_LENGTH_CLASSES", "k"), ("DD_READ_BOUND", "100")]:
        with env(**{k: v}):
            length_classes("r%d %s" % (i, k), pb, skip, params(5))

# ---- window screens ----
rng = np.random.default_rng(9)


def seq(n):
    return "".join(rng.choice(list("ACGT"), n))


def rd(n):
    return ReadRec(seq(n), [0.99] * n, 0.99, 1000)


odd = "".join(chr(c) for c in range(97, 97 + 29) if chr(c) not in "acgtn")
odd_windows = [Window(1000, ["ACGT" + odd], [rd(6)]), Window(1000, ["ACGT!#"], [rd(6)]), Window(1000, ["ACGT~"], [rd(6)]),
               Window(1000, ["AC~GT", "ACGT"], [rd(6)])]
shapes = [Window(1000, [seq(100), seq(130)], [rd(80)]), Window(1000, [seq(767), seq(50)], [rd(40)]), Window(1000, [seq(60)], [rd(1025), rd(30)]),
          Window(1000, [seq(60)], [ReadRec("", [], 0.99, 1000)]), Window(1000, [seq(766)], [rd(1024)]), Window(1000, [], [rd(50)]),
          Window(1000, [seq(70)], []), Window(1000, [seq(4094)], [rd(4096)]), Window(1000, [seq(4095)], [rd(100)]), Window(1000, [seq(100)], [rd(4097)]),
          Window(1000, ["", seq(40)], [rd(30)]), Window(1000, [seq(575)], [rd(100)]), Window(1000, [seq(574), seq(640)], [rd(100)]),
          Window(1000, [seq(766)], [rd(90)]), Window(1000, [seq(2000), seq(90)], [rd(1500), rd(70)])]
screens = {"shapes": pack(shapes), "odd": pack(shapes[:2] + odd_windows + shapes[11:]), "few-odd": pack(odd_windows[:2] + shapes[:1]),
           "ragged": ragged[0]}
for tag, pb in screens.items():
    b = pb.ctypes_batch()
    cl = np.full(pb.n_windows, 7, np.uint8)
    m2, m4 = (C.c_int32 * 2)(), (C.c_int32 * 4)()
    rc = lib.dd_screen_windows(C.byref(b), cl.ctypes.data_as(capi.c_u8p), C.byref(m2))
    rec("screen", tag, rc, cl.tolist(), list(m2))
    rec("screen null-max", tag, lib.dd_screen_windows(C.byref(b), cl.ctypes.data_as(capi.c_u8p), None), cl.tolist())
    for mld in (5, 12):
        for opt in (0, 1, 2, 3, 4):
            cl[:] = 7
            rc = lib.dd_screen_windows_ex(C.byref(params(mld)), C.byref(b), opt, cl.ctypes.data_as(capi.c_u8p), C.byref(m4))
            rec("screen-ex", tag, mld, opt, rc, err() if rc < 0 else "", cl.tolist(), list(m4) if rc >= 0 else "")
    rec("screen-ex null-params", tag, lib.dd_screen_windows_ex(None, C.byref(b), 1, cl.ctypes.data_as(capi.c_u8p), C.byref(m4)), err())
    rec("screen-ex opt0 null-params", tag, lib.dd_screen_windows_ex(None, C.byref(b), 0, cl.ctypes.data_as(capi.c_u8p), None), cl.tolist())

# ---- sizes, offsets, index, partition, pair-sum offsets, symbols ----
libs = [(np.array([0.1, 0.2, 0.3, 0.4]), 0.3), (np.array([1.0]), 1.0)]
with_libs = pack(shapes[:1] * 3, libraries=libs)
batches = dict(screens, uniform=synth.generate(12, H=5, R=30, L=100, hap_len=120, seed=3), libs=with_libs)
for tag, pb in batches.items():
    b = pb.ctypes_batch()
    W = pb.n_windows
    sz = capi.dd_sizes()
    rc = lib.dd_batch_sizes(C.byref(b), C.byref(sz))
    rec("sizes", tag, rc, *[getattr(sz, f) for f, _ in capi.dd_sizes._fields_])
    po, ho, vo = (np.full(W + 1, -1, np.int64) for _ in range(3))
    hw = np.full(max(pb.n_haps, 1), -1, np.int32)
    p64 = lambda a: a.ctypes.data_as(capi.c_i64p)
    rec("offsets", tag, lib.dd_batch_offsets(C.byref(b), p64(po), p64(ho), p64(vo)), digest(po), digest(ho), digest(vo), po[-1], ho[-1], vo[-1])
    rec("offsets partial", tag, lib.dd_batch_offsets(C.byref(b), None, p64(ho), None), digest(ho))
    po[:] = -1
    rec("index", tag, lib.dd_build_index(C.byref(b), hw.ctypes.data_as(capi.c_i32p), p64(po), p64(ho), p64(vo)), digest(hw), digest(po))
    for n in (1, 2, 3, 8):
        bd = np.full(n + 1, -1, np.int32)
        rec("partition", tag, n, lib.dd_partition_windows(C.byref(b), n, bd.ctypes.data_as(capi.c_i32p)), bd.tolist())
    hh = np.full(W + 1, -1, np.int64)
    rec("hh", tag, lib.dd_pair_sum_offsets(C.byref(b), p64(hh)), digest(hh), hh[-1])
    lut = np.zeros(256, np.uint8)
    rec("lut", tag, lib.dd_build_symbol_lut(C.byref(b), lut.ctypes.data_as(C.POINTER(C.c_uint8))), digest(lut))
lp, l95 = np.zeros(5), np.zeros(2)
f64 = lambda a: a.ctypes.data_as(capi.c_f64p)
rec("libtables", lib.dd_build_library_tables(C.byref(with_libs.ctypes_batch()), f64(lp), f64(l95)), lp.tobytes().hex(), l95.tobytes().hex())
for tag, bad in [("zero-prob", [(np.array([0.5, 0.0]), 0.5)]), ("zero-p95", [(np.array([0.5, 0.5]), 0.0)])]:
    rec("libtables", tag, lib.dd_build_library_tables(C.byref(pack(shapes[:1], libraries=bad).ctypes_batch()), f64(lp), f64(l95)), err())
rec("libtables no-libs", lib.dd_build_library_tables(C.byref(screens["shapes"].ctypes_batch()), f64(lp), f64(l95)), err())

# ---- the host tables, as raw bytes ----
quals = np.array([0.0, 0.5, 0.9, 0.99, 0.999, 0.9999, 1.0 - 1e-10, 1.0])
mapqs = np.array([0.0, 0.9, 0.99, 0.9999, 1.0 - 1e-9, 1.0 - 1e-12])
for tag, p in [("cli", params()), ("struct", params(cli=False)), ("mld31", params(31)), ("mqt30", capi.dd_params.from_dict(dict(params().as_dict(), mapQualThreshold=30.0)))]:
    t = np.zeros(capi.DD_TABLE_DOUBLES)
    rec("tables", tag, lib.dd_build_tables(C.byref(p), f64(quals), len(quals), f64(mapqs), len(mapqs), f64(t)), hashlib.sha1(t.tobytes()).hexdigest())
    rec("tables-empty", tag, lib.dd_build_tables(C.byref(p), None, 0, None, 0, f64(t)), hashlib.sha1(t.tobytes()).hexdigest())
t = np.zeros(capi.DD_TABLE_DOUBLES)
rec("tables too-many", lib.dd_build_tables(C.byref(params()), f64(quals), 257, f64(mapqs), 1, f64(t)), err())
for tag, kw in [("pError0", dict(pError=0.0)), ("pError1", dict(pError=1.0)), ("mld32", dict(maxLengthDel=32)), ("mld-1", dict(maxLengthDel=-1)),
                ("force", dict(forceReadOnHaplotype=1))]:
    p = capi.dd_params.from_dict(dict(params().as_dict(), **kw))
    rec("tables refused", tag, lib.dd_build_tables(C.byref(p), f64(quals), len(quals), f64(mapqs), len(mapqs), f64(t)), err())

# ---- refusals of the entry points (all before any device work) ----
one = synth.generate(1, H=2, R=3, L=50, hap_len=60, seed=5)
b = one.ctypes_batch()
arrs, res = alloc_result(one)
for tag, kw in [("mapUnmappedReads", dict(mapUnmappedReads=1)), ("force", dict(forceReadOnHaplotype=1)), ("mld32", dict(maxLengthDel=32))]:
    p = capi.dd_params.from_dict(dict(params().as_dict(), **kw))
    for fn in ("dd_compute_likelihoods", "dd_compute_likelihoods_faster"):
        if tag == "mapUnmappedReads" and fn.endswith("faster"):
            continue                                     # (the --faster model ignores the switch and would go on to the device)
        rec("refused", fn, tag, getattr(lib, fn)(C.byref(p), C.byref(b), C.byref(res), 0), err())
rec("refused no-outputs", lib.dd_compute_likelihoods(C.byref(params()), C.byref(b), C.byref(capi.dd_result()), 0), err())
rec("refused null-params", lib.dd_compute_likelihoods(None, C.byref(b), C.byref(res), 0), err())
rec("refused option-bits", lib.dd_compute_likelihoods_ex(C.byref(params()), C.byref(b), C.byref(res), 0, 2), err(),
    lib.dd_compute_likelihoods_faster_ex(C.byref(params()), C.byref(b), C.byref(res), 0, 1), err())
dev = (C.c_int32 * 1)(0)
rec("refused multi no-devices", lib.dd_compute_likelihoods_multi(C.byref(params()), C.byref(b), C.byref(res), dev, 0), err())
nb = one.ctypes_batch()
nb.hap_seq_off = None
sz = capi.dd_sizes()
cl = np.zeros(4, np.uint8)
bd = np.zeros(4, np.int32)
rec("null-offsets", lib.dd_batch_sizes(C.byref(nb), C.byref(sz)), err(), lib.dd_screen_windows(C.byref(nb), cl.ctypes.data_as(capi.c_u8p), None), err(),
    lib.dd_screen_windows_ex(C.byref(params()), C.byref(nb), 1, cl.ctypes.data_as(capi.c_u8p), None), err(),
    lib.dd_partition_windows(C.byref(nb), 2, bd.ctypes.data_as(capi.c_i32p)), err())
rec("null-args", lib.dd_batch_sizes(None, C.byref(sz)), err(), lib.dd_screen_windows(C.byref(b), None, None), err(),
    lib.dd_partition_windows(C.byref(b), 0, bd.ctypes.data_as(capi.c_i32p)), err(), lib.dd_pair_sum_offsets(C.byref(b), None), err(),
    lib.dd_batch_offsets(None, None, None, None), err(), lib.dd_build_length_classes(C.byref(b), None, None, None, None), err())
unsorted = one.ctypes_batch()
bad_off = one.a["hap_seq_off"].copy()
bad_off[1] = bad_off[2] + 5
unsorted.hap_seq_off = bad_off.ctypes.data_as(capi.c_i32p)
rec("not-monotone", lib.dd_batch_sizes(C.byref(unsorted), C.byref(sz)), err())
too_long = pack([shapes[1]])
lc = capi.dd_length_classes()
lst = np.zeros(too_long.n_haps * capi.N_READ_CLASSES + 1, np.int32)
rec("classes unflagged-long", lib.dd_build_length_classes(C.byref(too_long.ctypes_batch()), None, C.byref(params()), lst.ctypes.data_as(capi.c_i32p), C.byref(lc)), err())

with open(sys.argv[1], "w") as f:
    f.write("\n".join(out) + "\n")
print("host_equivalence: %d records -> %s" % (len(out), sys.argv[1]))
