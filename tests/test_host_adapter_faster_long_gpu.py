"""GPU: the C++ adapter with LikelihoodEngine::setLongWindowsFaster(true) — a window with a 767-bp haplotype (beyond dd_faster_kernel)
computed through computeLikelihoodsFaster (eager records) and computeLikelihoodsBatch (lazy views, with and without the alignments kept),
equal to the oracle's --faster model; setLongWindows(true) alone changes nothing for that model."""
import numpy as np
import pytest

from dindel_tgi_amd import capi
from dindel_tgi_amd.batch import ReadRec, Window, pack
from tests import _host, _oracle
from tests.test_host_adapter_long_gpu import _batch_json, _call, _window

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mld", [5, 20])
def test_engine_faster_long_window_equals_oracle(mld):
    p = capi.params_cli_defaults()
    p.maxLengthDel = mld
    haps, reads, quals, starts = _window(mld)
    _host.load().ddh_compute_window_faster_long_json.argtypes = _host.load().ddh_compute_window_long_json.argtypes
    got = _call("ddh_compute_window_faster_long_json", haps, reads, quals, starts, p)
    assert "throw" not in got, got
    pb = pack([Window(1000, haps, [ReadRec(r, [q] * len(r), 0.9999, s) for r, q, s in zip(reads, quals, starts)])])
    want = _oracle.batch(p, pb, nthreads=8, faster=True)
    assert (want["status"][:pb.n_pairs] == 0).all()
    R = len(reads)
    for h in range(len(haps)):
        for r in range(R):
            ml, i = got["liks"][h][r], h * R + r
            assert ml["ll"] == want["ll"][i] and ml["llOn"] == want["llOn"][i] and ml["llOff"] == want["llOff"][i], (h, r)
            for k in ("offHap", "offHapHMQ", "numIndels", "numMismatch", "firstBase", "lastBase"):
                assert ml[k] == int(want[k][i]), (h, r, k)
            assert ml["hpos"] == capi.hpos_reference_codes(want["hpos"][h * pb.hpos_len // len(haps) + sum(len(x) for x in reads[:r]):][:len(reads[r])]).tolist()
    assert got["onHap"] == [int(v) for v in want["onHap"][:R]]
    # without the option the adapter reports the window as one that threw, as before
    plain = _call("ddh_compute_window_faster_json", haps, reads, quals, starts, p)
    assert "throw" in plain and "outside the GPU kernel limits" in plain["throw"]


@pytest.mark.parametrize("keep_alignments", [True, False])
def test_engine_lazy_views_of_a_faster_long_window(keep_alignments):
    p = capi.params_cli_defaults()
    haps, reads, quals, starts = _window(7)
    long_w = Window(1000, haps, [ReadRec(r, [q] * len(r), 0.9999, s) for r, q, s in zip(reads, quals, starts)])
    rng = np.random.default_rng(3)
    h = "".join(rng.choice(list("ACGT"), 150))
    short_w = Window(1000, [h, h[:70] + h[72:]], [ReadRec(h[o:o + 100], [0.999] * 100, 0.9999, 1000 + o) for o in range(0, 50, 5)])
    flags = 1 | 8 | (0 if keep_alignments else 2)
    got = _batch_json([short_w, long_w], p, flags)
    assert got["mismatch"] == 0
    assert [w["error"] for w in got["windows"]] == ["", ""]
    want = _oracle.batch(p, pack([short_w, long_w]), nthreads=8, faster=True)
    n0 = len(short_w.haps) * len(short_w.reads)
    assert got["windows"][1]["ll"] == [float(v) for v in want["ll"][n0:]]
    assert got["windows"][1]["onHap"] == [int(v) for v in want["onHap"][len(short_w.reads):]]
    plain = _batch_json([short_w, long_w], p, flags & ~8)
    assert plain["windows"][0]["ll"] == got["windows"][0]["ll"]
    assert plain["windows"][1]["error"].startswith("window outside the GPU kernel limits")
    # setLongWindows(true) alone changes nothing for the --faster model
    main_opt = _batch_json([short_w, long_w], p, (flags & ~8) | 4)
    assert main_opt == plain
