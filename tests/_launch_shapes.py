"""The cases of tests/golden/launch_shapes.json: batches built from a recipe, the scalars a launch is shaped from, and a run of one case.

A case is dict(name, recipe, params, maxLengthDel, env, entry, asks, last_launch, kernel_name).  `recipe` is a list of synth.generate keyword
sets ("tile": n repeats that part's windows n times); `entry` is "device" (DeviceBatch.launch), "device_faster" (launch_faster) or "host"
(dd_compute_likelihoods).  `asks` holds, for every launch the entry point shapes, the scalars plan.cpp's shape_launch / shape_fast is asked
with (ASK_FIELDS, in the order of the calls) and the dd_launch_log record it left (without the duration; None where nothing was launched:
an empty range, or the --faster kernel, which keeps no log).  tests/test_launch_shape_cpu.py feeds the scalars to the shape functions on
their own; tests/test_gpu_launch_shapes.py runs some of the recipes."""
import ctypes as C
import json
import os

import numpy as np

from dindel_tgi_amd import capi, synth

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_shapes.json")
# the fields of ddh::LaunchAsk besides the parameters, in the order tests/launch_shape_check.cpp reads them
ASK_FIELDS = ["faster", "n_windows", "n_haps", "n_reads", "max_hap_len", "max_read_len", "n_qual", "max_window_reads",
              "has_class", "has_list", "list_begin", "list_end", "cls_max_hap_len", "cls_max_read_len", "cls_min_read_len",
              "cls_max_window_reads", "cls_avg_window_reads", "cls_avg_read_len", "hap_begin", "hap_end", "workspace_bytes", "overlapping_chunks"]
US = capi.LAUNCH_LOG_FIELDS.index("us")


def load_cases():
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


def build_batch(recipe):
    """The batch of a recipe and, per part, (the part before tiling, its repeats): the oracle runs on the former."""
    parts, bases = [], []
    for part in recipe:
        kw = dict(part)
        reps = kw.pop("tile", 1)
        base = synth.generate(kw.pop("n"), **kw)
        bases.append((base, reps))
        parts.append(synth.tile(base, reps) if reps > 1 else base)
    return (parts[0] if len(parts) == 1 else synth.concat(parts)), bases


def params_of(case):
    p = capi.params_struct_defaults() if case["params"] == "struct" else capi.params_cli_defaults()
    if case.get("maxLengthDel") is not None:
        p.maxLengthDel = case["maxLengthDel"]
    return p


def _ask(faster, db, cls, list_range, hap_range, ws_bytes, overlapping):
    a = dict.fromkeys(ASK_FIELDS, 0)
    a.update(faster=int(faster), n_windows=db.n_windows, n_haps=db.n_haps, n_reads=db.n_reads, max_hap_len=db.max_hap_len,
             max_read_len=db.max_read_len, n_qual=db.n_qual, max_window_reads=db.max_window_reads, hap_begin=hap_range[0], hap_end=hap_range[1],
             workspace_bytes=int(ws_bytes), overlapping_chunks=int(overlapping), cls_min_read_len=1)
    if cls is not None:
        a.update(has_class=1, has_list=1, list_begin=list_range[0], list_end=list_range[1], cls_max_hap_len=cls.max_hap_len,
                 cls_max_read_len=cls.max_read_len, cls_min_read_len=cls.min_read_len, cls_max_window_reads=cls.max_window_reads,
                 cls_avg_window_reads=cls.avg_window_reads, cls_avg_read_len=cls.avg_read_len)
    return a


def device_asks(dev, faster):
    """What dd_launch_device / dd_launch_device_faster shape for a resident batch (launch.cpp)."""
    if faster:
        return [_ask(True, dev.db, None, None, (0, -1), 0, False)]
    n = dev.classes.n_launches
    if n > 1:
        return [_ask(False, dev.db, dev.classes.launch[i], (0, dev.classes.launch[i].list_len), (0, dev.db.n_haps), dev.ws_bytes, False) for i in range(n)]
    return [_ask(False, dev.db, None, None, (0, -1), dev.ws_bytes, False)]


def host_asks(lib, p, pb):
    """What dd_compute_likelihoods shapes for a batch in pageable memory: host_path.cpp's plan and window blocks, restated for batches
    without screened windows and well away from the 64 MB staging limit."""
    hb = pb.ctypes_batch()
    skip = np.zeros(max(pb.n_windows, 1), np.uint8)
    mx = (C.c_int32 * 2)()
    assert lib.dd_screen_windows(C.byref(hb), skip.ctypes.data_as(capi.c_u8p), C.byref(mx)) == 0, "a recipe with screened windows"
    cls = capi.dd_length_classes()
    lst = np.zeros(max(pb.n_haps, 1) * capi.N_READ_CLASSES + 1, np.int32)
    assert lib.dd_build_length_classes(C.byref(hb), None, C.byref(p), lst.ctypes.data_as(capi.c_i32p), C.byref(cls)) == 0, capi.last_error()
    db = capi.dd_device_batch()
    db.n_windows, db.n_haps, db.n_reads = pb.n_windows, pb.n_haps, pb.n_reads
    db.max_hap_len, db.max_read_len = max(int(mx[0]), 1), max(int(mx[1]), 1)
    db.n_qual, db.n_mapq = hb.n_qual, hb.n_mapq
    db.max_window_reads = int(np.diff(pb.a["win_read_off"]).max())
    ws_bytes = int(lib.dd_workspace_bytes(C.byref(p), C.byref(db)))
    single = cls.n_launches <= 1
    if not single:
        db.classes, db.hap_class_list = C.addressof(cls), lst.ctypes.data
        ws_bytes = max(ws_bytes, int(lib.dd_workspace_bytes(C.byref(p), C.byref(db))))
        db.classes, db.hap_class_list = None, None
    from dindel_tgi_amd.batch import RESULT_DTYPES, result_lengths
    out_bytes = sum(n * np.dtype(RESULT_DTYPES[k]).itemsize for k, n in result_lengths(pb).items())
    assert out_bytes < (48 << 20) or out_bytes > (64 << 20), "a recipe too close to the staging limit to restate the block count"
    n_chunks = 1 if out_bytes <= (64 << 20) else max(1, min(64, pb.n_windows, (pb.n_pairs + 999999) // 1000000))
    cw = [0]
    for c in range(1, n_chunks):
        w = cw[-1]
        while w < pb.n_windows and pb.win_pair_off[w] < pb.n_pairs * c // n_chunks:
            w += 1
        cw.append(w)
    cw.append(pb.n_windows)
    asks = []
    for c in range(n_chunks):
        g0, g1 = int(pb.a["win_hap_off"][cw[c]]), int(pb.a["win_hap_off"][cw[c + 1]])
        if single:
            asks.append(_ask(False, db, None, None, (g0, g1), ws_bytes, n_chunks > 1))
            continue
        for i in range(cls.n_launches):
            L = cls.launch[i]
            hl = lst[L.list_off:L.list_off + L.list_len]
            rng = (int(np.searchsorted(hl, g0, "left")), int(np.searchsorted(hl, g1, "left")))
            asks.append(_ask(False, db, L, rng, (g0, g1), ws_bytes, n_chunks > 1))
    return asks


def launches(ask):
    """Whether the launch an ask describes covers any haplotype (an empty one leaves no record)."""
    if ask["has_list"]:
        return ask["list_end"] > ask["list_begin"]
    return ask["hap_end"] < 0 or ask["hap_end"] > ask["hap_begin"]


def run_case(lib, case):
    """Run a case's recipe through its entry point under its switches.  Returns (asks, records without the duration, last_launch as a list,
    kernel name, results, batch, bases)."""
    import torch
    from dindel_tgi_amd.device import DeviceBatch
    from tests.test_gpu_parity import run_host_api
    pb, bases = build_batch(case["recipe"])
    p = params_of(case)
    old = {k: os.environ.get(k) for k in case["env"]}
    os.environ.update(case["env"])
    try:
        if case["entry"] == "host":
            asks = host_asks(lib, p, pb)
            got = run_host_api(lib, p, pb)
        else:
            faster = case["entry"] == "device_faster"
            dev = DeviceBatch(pb, p, "cuda:0")
            asks = device_asks(dev, faster)
            (dev.launch_faster if faster else dev.launch)()
            torch.cuda.synchronize()
            got = dev.results()
        log = [[r[k] for k in capi.LAUNCH_LOG_FIELDS if k != "us"] for r in capi.launch_log()] if case["entry"] != "device_faster" else []
        last = list(capi.last_launch().values())
        name = lib.dd_kernel_name().decode()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    return asks, log, last, name, got, pb, bases
