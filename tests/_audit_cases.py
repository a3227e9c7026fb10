"""What the audit's tests share (helper; no tests in here): a restatement of the comparison rule in numpy, written unlike
csrc/audit_kernel.h's loop (masks over whole arrays instead of a walk over pairs), and dd_result structs over host arrays.

The rule (include/dindel_hmm.h, "audit"): status first; equal statuses OK / NAN / LLPOS open the 14 per-pair values, the pair's hpos, its
var_covered and, with hap_var_flank, its var_fcov; HAPSIZE opens ll and the coverage flags; anything else nothing more."""
import ctypes as C
import functools

import numpy as np

from dindel_tgi_amd import capi
from tests import _path_scenarios as ps

PER_ELEMENT = ("hpos", "var_covered", "var_fcov")
PAIR_VALUES = capi.AUDIT_FIELDS[1:15]
COMPUTED = (capi.DD_PAIR_OK, capi.DD_PAIR_NAN, capi.DD_PAIR_LLPOS)


def result_struct(arrs, null=()):
    """A dd_result over host arrays, the fields in `null` (and onHap when absent) NULL."""
    res = capi.dd_result()
    for k, typ in capi.RESULT_FIELDS:
        if k in arrs and k not in null:
            setattr(res, k, arrs[k].ctypes.data_as(typ))
    return res


def window_of_pairs(pb):
    return np.repeat(np.arange(pb.n_windows), np.diff(pb.win_pair_off))


def expected_compared(pb, status, chosen, has_flank):
    """-> {field: elements an audit of the windows `chosen` compares}, from the pairs' statuses (both sides equal) and the rule."""
    st = np.asarray(status[:pb.n_pairs])
    in_sample = np.isin(window_of_pairs(pb), chosen)
    computed = in_sample & np.isin(st, COMPUTED)
    cov = in_sample & (np.isin(st, COMPUTED) | (st == capi.DD_PAIR_HAPSIZE))
    elem = ps.element_pairs(pb)
    out = {"status": int(in_sample.sum()), "ll": int(cov.sum())}
    for k in PAIR_VALUES[1:]:
        out[k] = int(computed.sum())
    out["hpos"] = int(computed[elem["hpos"][:pb.hpos_len]].sum())
    out["var_covered"] = int(cov[elem["var_covered"][:pb.var_cov_len]].sum())
    out["var_fcov"] = out["var_covered"] if has_flank else 0
    return out


def shadow_slices(pb, sample):
    """Per chosen window: (window, slice of the per-pair arrays, of hpos, of the coverage arrays) in the PRIMARY; the shadow holds the same
    pieces back to back, in window order."""
    out = []
    for w in sample.chosen:
        w = int(w)
        out.append((w, slice(int(pb.win_pair_off[w]), int(pb.win_pair_off[w + 1])), slice(int(pb.win_hpos_off[w]), int(pb.win_hpos_off[w + 1])),
                    slice(int(pb.win_varcov_off[w]), int(pb.win_varcov_off[w + 1]))))
    return out


def shadow_from(pb, sample, arrs):
    """The shadow a correct recomputation would leave: the chosen windows' pieces of `arrs`, compacted."""
    sl = shadow_slices(pb, sample)
    out = {}
    for k, _t in capi.RESULT_FIELDS:
        if k == "onHap":
            continue
        i = 2 if k == "hpos" else 3 if k in ("var_covered", "var_fcov") else 1
        parts = [np.asarray(arrs[k])[s[i]] for s in sl]
        out[k] = np.concatenate(parts) if parts else np.zeros(0, np.asarray(arrs[k]).dtype)
        if out[k].size == 0:
            out[k] = np.zeros(1, out[k].dtype)
    return out


@functools.lru_cache(maxsize=None)
def scenario(hap_len=126, read_len=36, mld=5):
    """(PackedBatch, index, params, oracle arrays) of a scenario batch: one oracle run, shared and left unchanged."""
    from tests import _oracle
    pb, index = ps.batch_for(hap_len, read_len, mld)
    p = ps.params_for(mld, 1)
    want = _oracle.batch(p, pb, nthreads=16)
    for a in want.values():
        a.setflags(write=False)
    return pb, index, p, want


def main_classes(lib, p, pb):
    """dd_screen_windows' bytes (0 = a window the main kernels compute)."""
    b = pb.ctypes_batch()
    skip = np.zeros(max(pb.n_windows, 1), np.uint8)
    mx = (C.c_int32 * 2)()
    assert lib.dd_screen_windows(C.byref(b), skip.ctypes.data_as(capi.c_u8p), C.byref(mx)) >= 0, capi.last_error()
    return skip[:pb.n_windows]
