"""The EM loop of the pooled analysis (estimateHaplotypeFrequenciesBayesEM) over slots = (window, set of active variants):
dd_pooled_em (device), dd_pooled_em_host (CPU) and dd_pooled_em_device on a resident batch (DeviceBatch.pooled_em).

The arithmetic is the library's (csrc/pooled_math.h: one definition for the kernel and the CPU evaluation, bit-equal outputs); there is
no Python implementation behind this module.  A batch is described by win_hap_off / win_read_off (int32 [n_windows + 1]) and `ll`, the
likelihood kernels' per-pair array (pair(w, h, r) = win_pair_off[w] + h * R_w + r); slots by slot_window (one window index per slot) and
compat (one sequence of H_w bytes per slot, 0 = incompatible).
"""
import ctypes as C

import numpy as np

from . import capi

MATH_FUNCTIONS = {"exp": 0, "log": 1, "digamma": 2, "add_logs": 3}


def _pad(arr):
    return arr if arr.size else np.zeros(1, arr.dtype)


def pack_slots(win_hap_off, slot_window, compat):
    """dict(slot_window int32 [n], slot_off int64 [n + 1], compat uint8 [slot_off[n]]) for dd_pooled_slots."""
    who = np.asarray(win_hap_off, np.int64)
    sw = np.ascontiguousarray(slot_window, np.int32)
    if len(compat) != len(sw):
        raise ValueError("one compat sequence per slot")
    if len(sw) and (sw.min() < 0 or sw.max() >= len(who) - 1):
        raise ValueError("slot_window names no window of the batch")
    nh = (who[1:] - who[:-1])[sw] if len(sw) else np.zeros(0, np.int64)
    for i, c in enumerate(compat):
        if len(c) != nh[i]:
            raise ValueError("slot %d: %d compat bytes for %d haplotypes" % (i, len(c), nh[i]))
    flat = np.concatenate([np.asarray(c, np.uint8) for c in compat]) if len(compat) else np.zeros(0, np.uint8)
    return {"slot_window": sw, "slot_off": np.concatenate([[0], np.cumsum(nh)]).astype(np.int64),
            "compat": np.ascontiguousarray(flat, np.uint8)}


def alloc_result(slots):
    n, f = len(slots["slot_window"]), int(slots["slot_off"][-1])
    return {"loglik": np.zeros(n), "freqs": np.zeros(f), "iters": np.zeros(n, np.int32), "ediff": np.zeros(n)}


def _structs(slots, res):
    s = capi.dd_pooled_slots(len(slots["slot_window"]), *[_pad(slots[k]).ctypes.data for k in ("slot_window", "slot_off", "compat")])
    keep = {k: _pad(res[k]) for k in capi.POOLED_RESULT_FIELDS}
    r = capi.dd_pooled_result(*[keep[k].ctypes.data for k in capi.POOLED_RESULT_FIELDS])
    return s, r, keep


def _batch(win_hap_off, win_read_off):
    b = capi.dd_batch()
    who, wro = np.ascontiguousarray(win_hap_off, np.int32), np.ascontiguousarray(win_read_off, np.int32)
    b.n_windows = len(who) - 1
    b.win_hap_off, b.win_read_off = who.ctypes.data_as(capi.c_i32p), wro.ctypes.data_as(capi.c_i32p)
    b._keep = (who, wro)
    return b


def _run(fn, name, win_hap_off, win_read_off, ll, slots, a0, tol, last):
    b = _batch(win_hap_off, win_read_off)
    llc = _pad(np.ascontiguousarray(ll, np.float64))
    res = alloc_result(slots)
    s, r, keep = _structs(slots, res)
    rc = fn(C.byref(b), llc.ctypes.data_as(capi.c_f64p), C.byref(s), a0, tol, C.byref(r), last)
    if rc != 0:
        raise RuntimeError("%s: %d %s" % (name, rc, capi.last_error()))
    return {k: keep[k][:len(res[k])] for k in res}


def em_host(win_hap_off, win_read_off, ll, slots, a0=0.001, tol=1e-4, nthreads=1):
    """dd_pooled_em_host: dict(loglik, freqs, iters, ediff); freqs of slot s at slots['slot_off'][s]."""
    return _run(capi.load().dd_pooled_em_host, "dd_pooled_em_host", win_hap_off, win_read_off, ll, slots, a0, tol, nthreads)


def em(win_hap_off, win_read_off, ll, slots, a0=0.001, tol=1e-4, device=0):
    """dd_pooled_em: the same on the device (host arrays in, host arrays out)."""
    return _run(capi.load().dd_pooled_em, "dd_pooled_em", win_hap_off, win_read_off, ll, slots, a0, tol, device)


def math_eval(fn, x):
    """pooled_math.h's exp / log / digamma over an array, or add_logs over an [n, 2] array (dd_pooled_math_eval, host)."""
    xs = np.ascontiguousarray(x, np.float64)
    n = xs.shape[0]
    y = np.zeros(max(n, 1))
    rc = capi.load().dd_pooled_math_eval(MATH_FUNCTIONS[fn], _pad(xs.reshape(-1)).ctypes.data_as(capi.c_f64p), y.ctypes.data_as(capi.c_f64p), n)
    if rc != 0:
        raise RuntimeError("dd_pooled_math_eval: %d %s" % (rc, capi.last_error()))
    return y[:n]
