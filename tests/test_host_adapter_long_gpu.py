"""GPU: the C++ adapter with LikelihoodEngine::setLongWindows(true) — a window with a 767-bp haplotype (beyond the main kernels) computed
through computeLikelihoods (eager records) and computeLikelihoodsBatch (lazy WindowLikelihoods views, with and without the alignments kept),
equal to the oracle; without the option the same window is reported as one that threw, as before."""
import numpy as np
import pytest

from dindel_tgi_amd import capi
from dindel_tgi_amd.batch import ReadRec, Window, pack
from tests import _host, _oracle

pytestmark = pytest.mark.gpu


def _window(seed):
    rng = np.random.default_rng(seed)
    ref = "".join(rng.choice(list("ACGT"), 767))
    haps = [ref, ref[:380] + ref[392:], ref[:380] + "GATTACA" + ref[380:]]
    reads, quals, starts = [], [], []
    for i in range(12):
        h = haps[i % 3]
        off = int(rng.integers(-40, len(h) - 60))
        seq = "".join(h[j] if 0 <= j < len(h) else rng.choice(list("ACGT")) for j in range(off, off + 120))
        reads.append(seq); quals.append(0.999 if i % 2 else 0.99); starts.append(1000 + off)
    return haps, reads, quals, starts


def _call(fn_name, haps, reads, quals, starts, p):
    import ctypes as C
    import json
    lib = _host.load()
    q = np.ascontiguousarray(np.concatenate([np.full(len(r), x) for x, r in zip(quals, reads)]))
    mq = np.full(len(reads), 0.9999); pf = np.asarray(starts, np.float64); um = np.zeros(len(reads), np.int32)
    pd, pi = _host._params(p)
    out = C.create_string_buffer(1 << 24)
    n = getattr(lib, fn_name)("\n".join(haps).encode(), "\n".join(reads).encode(), q.ctypes.data_as(capi.c_f64p),
                              mq.ctypes.data_as(capi.c_f64p), pf.ctypes.data_as(capi.c_f64p), um.ctypes.data_as(capi.c_i32p),
                              C.c_uint(1000), pd, pi, 0, out, len(out))
    assert n > 0, n
    return json.loads(out.value.decode())


@pytest.mark.parametrize("mld", [5, 20])
def test_engine_long_window_equals_oracle(mld):
    p = capi.params_cli_defaults()
    p.maxLengthDel = mld
    haps, reads, quals, starts = _window(mld)
    got = _call("ddh_compute_window_long_json", haps, reads, quals, starts, p)
    assert "throw" not in got, got
    pb = pack([Window(1000, haps, [ReadRec(r, [q] * len(r), 0.9999, s) for r, q, s in zip(reads, quals, starts)])])
    want = _oracle.batch(p, pb, nthreads=8)
    R = len(reads)
    for h in range(len(haps)):
        for r in range(R):
            ml, i = got["liks"][h][r], h * R + r
            assert ml["ll"] == want["ll"][i] and ml["llOn"] == want["llOn"][i] and ml["llOff"] == want["llOff"][i], (h, r)
            for k in ("offHap", "offHapHMQ", "numIndels", "numMismatch", "nBQT", "nmmBQT", "nMMLeft", "nMMRight", "firstBase", "lastBase"):
                assert ml[k] == int(want[k][i]), (h, r, k)
            assert ml["hpos"] == capi.hpos_reference_codes(want["hpos"][h * pb.hpos_len // len(haps) + sum(len(x) for x in reads[:r]):][:len(reads[r])]).tolist()
    assert got["onHap"] == [int(v) for v in want["onHap"][:R]]
    # without the option the adapter reports the window as one that threw (the reference's skipped row), as before
    plain = _call("ddh_compute_window_json", haps, reads, quals, starts, p)
    assert "throw" in plain and "outside the GPU kernel limits" in plain["throw"]


def _batch_json(windows, p, flags):
    import ctypes as C
    import json
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
    pd, pi = _host._params(p)
    out = C.create_string_buffer(1 << 26)
    n = lib.ddh_batch_json(len(windows), nh.ctypes.data_as(capi.c_i32p), nr.ctypes.data_as(capi.c_i32p), "\n".join(haps).encode(),
                           "\n".join(r.seq for r in reads).encode(), q.ctypes.data_as(capi.c_f64p), mq.ctypes.data_as(capi.c_f64p),
                           pf.ctypes.data_as(capi.c_f64p), um.ctypes.data_as(capi.c_i32p), lp.ctypes.data_as(capi.c_u32p), pd, pi, flags, 0,
                           out, len(out))
    assert n > 0, n
    return json.loads(out.value.decode())


@pytest.mark.parametrize("keep_alignments", [True, False])
def test_engine_lazy_views_of_a_long_window(keep_alignments):
    """computeLikelihoodsBatch with long windows on: the lazy views (every scalar accessor and get()) equal the eager records, the ll of
    the long window equals the oracle, and the ordinary window beside it gives the same ll as without the option."""
    p = capi.params_cli_defaults()
    haps, reads, quals, starts = _window(7)
    long_w = Window(1000, haps, [ReadRec(r, [q] * len(r), 0.9999, s) for r, q, s in zip(reads, quals, starts)])
    rng = np.random.default_rng(3)
    h = "".join(rng.choice(list("ACGT"), 150))
    short_w = Window(1000, [h, h[:70] + h[72:]], [ReadRec(h[o:o + 100], [0.999] * 100, 0.9999, 1000 + o) for o in range(0, 50, 5)])
    flags = 4 | (0 if keep_alignments else 2)
    got = _batch_json([short_w, long_w], p, flags)
    assert got["mismatch"] == 0
    assert [w["error"] for w in got["windows"]] == ["", ""]
    want = _oracle.batch(p, pack([short_w, long_w]), nthreads=8)
    n0 = len(short_w.haps) * len(short_w.reads)
    assert got["windows"][1]["ll"] == [float(v) for v in want["ll"][n0:]]
    assert got["windows"][1]["onHap"] == [int(v) for v in want["onHap"][len(short_w.reads):]]
    plain = _batch_json([short_w, long_w], p, flags & ~4)
    assert plain["windows"][0]["ll"] == got["windows"][0]["ll"]
    assert plain["windows"][1]["error"].startswith("window outside the GPU kernel limits")
