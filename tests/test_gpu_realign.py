"""GPU: the realigned reads on the device (dd_realign_device / dd_compute_likelihoods_realign, realign_kernel.hip): per read the haplotype
it is realigned to and that pair's CIGAR.  Exact equality, three ways: the chosen haplotype against a numpy restatement of the two rules
(below), the CIGAR against the host specification (dindel::getCIGAR through ddh_get_cigar) for the chosen pair, and the whole row against
the row dd_cigars_device gives for that same pair on the same arrays.

The entry takes ll, onHap, status and hpos as pointers, so most cases feed it hand-made ones; output arrays start out filled with a
pattern, so a word the kernel must not write is seen if it does."""
import ctypes as C

import numpy as np
import pytest
import torch

from dindel_tgi_amd import capi, synth
from dindel_tgi_amd.batch import ReadRec, Window, alloc_result, pack
from dindel_tgi_amd.device import DeviceBatch
from tests import _cigar_cases as cc
from tests.test_gpu_cigars import assert_same_bytes, with_page_locked_results

pytestmark = pytest.mark.gpu
FILL = 0x3B3B3B3B
FIRST_MAX, PAIR = capi.DD_REALIGN_FIRST_MAX, capi.DD_REALIGN_PAIR
INF, NAN = np.inf, np.nan
HAP_LEN = 200


# ---------------------------------------------------------------- the two rules, restated
def choose(pb, mode, ll, on_hap=None, pairs=None, n_indels=None):
    """-> (hap [n_reads]: the chosen haplotype or -1, none [n_reads]: the DD_REALIGN_* status where nothing is chosen, pair [n_reads])."""
    a = pb.a
    hap, none, pair = np.full(pb.n_reads, -1, np.int32), np.zeros(pb.n_reads, np.int32), np.full(pb.n_reads, -1, np.int64)
    for w in range(pb.n_windows):
        g0, q0 = int(a["win_hap_off"][w]), int(a["win_read_off"][w])
        H, R = int(a["win_hap_off"][w + 1]) - g0, int(a["win_read_off"][w + 1]) - q0
        p0 = int(pb.win_pair_off[w])
        for r in range(R):
            q = q0 + r
            if H == 0:
                none[q] = capi.DD_REALIGN_NO_HAPS
                continue
            col = ll[p0 + r:p0 + H * R:R]
            assert len(col) == H
            if mode == FIRST_MAX:
                if on_hap is not None and not on_hap[q]:
                    none[q] = capi.DD_REALIGN_OFF_HAP
                    continue
                best, hidx = -INF, 0
                for h in range(H):                                   # DInDel.cpp:505-510
                    if col[h] > best:
                        best, hidx = col[h], h
            else:
                h1, h2 = int(pairs[2 * w]), int(pairs[2 * w + 1])
                if not (0 <= h1 < H and 0 <= h2 < H):
                    none[q] = capi.DD_REALIGN_BAD_PAIR
                    continue
                with np.errstate(invalid="ignore"):
                    close = np.abs(np.float64(col[h1]) - np.float64(col[h2])) < 1e-8    # DInDel.cpp:598
                if close:
                    hidx = h1 if n_indels[g0 + h1] < n_indels[g0 + h2] else h2
                else:
                    hidx = h1 if col[h1] > col[h2] else h2
            hap[q], pair[q] = hidx, p0 + hidx * R + r
    return hap, none, pair


def host_rows(pb, pair, hpos, hap_ref_pos, hap_aligned, pair_status, ops_cap):
    """What the walk must leave for the chosen pairs, per READ, from ddh_get_cigar; reads without a pair keep the fill."""
    hso = pb.a["hap_seq_off"]
    codes = capi.hpos_reference_codes(hpos)
    n = pb.n_reads
    want = dict(n_ops=np.full(n, FILL, np.int32), ops=np.full((n, ops_cap), FILL, np.uint32), ref_off=np.full(n, FILL, np.int32), status=np.full(n, FILL, np.int32))
    where = {int(p): q for q, p in enumerate(pair) if p >= 0}
    for p, g, sl in cc.pair_hpos_slices(pb):
        q = where.get(p)
        if q is None:
            continue
        if pair_status is not None and pair_status[p] != 0:
            want["status"][q], want["n_ops"][q], want["ref_off"][q] = capi.DD_CIGAR_NOT_COMPUTED, 0, -1
            continue
        res = -1 if hap_aligned is not None and not hap_aligned[g] else cc.host_cigar(hap_ref_pos[hso[g]:hso[g + 1]], codes[sl])
        if isinstance(res, int):
            want["status"][q], want["n_ops"][q], want["ref_off"][q] = cc.HOST_CODE_TO_STATUS[res], 0, -1
            continue
        cig, ref_pos = res
        want["n_ops"][q], want["ref_off"][q] = len(cig), ref_pos
        want["status"][q] = capi.DD_CIGAR_OVERFLOW if len(cig) > ops_cap else capi.DD_CIGAR_OK
        for i, (op, ln) in enumerate(cig[:ops_cap]):
            want["ops"][q, i] = (ln << 4) | op
    return want


def run(pb, hap_ref_pos, mode=FIRST_MAX, hap_aligned=None, ops_cap=8, ll=None, on_hap=None, hpos=None, status=None, pairs=None, n_indels=None,
        launch=None, use_on_hap=True, **kw):
    """DeviceBatch(cigars=True, realign=True): the likelihood launch (or the given arrays instead), then both CIGAR launches -> results()."""
    dev = DeviceBatch(pb, capi.params_cli_defaults(), "cuda:0", cigars=True, realign=True, ops_cap=ops_cap, hap_ref_pos=hap_ref_pos,
                      hap_aligned=hap_aligned, hap_n_indels=n_indels, **kw)
    if launch == "main":
        dev.launch()
    elif launch == "faster":
        dev.launch_faster()
    for name, arr, dt in (("ll", ll, np.float64), ("onHap", on_hap, np.uint8), ("hpos", hpos, np.int16), ("status", status, np.int32)):
        if arr is not None and len(arr):
            dev.out[name][:len(arr)] = torch.from_numpy(np.ascontiguousarray(arr, dt)).to(dev.device)
    for t in list(dev.cig.values()) + list(dev.rl.values()):
        t.fill_(FILL)
    dev.launch_cigars()
    dev.launch_realign(mode, win_hap_pair=pairs, on_hap=use_on_hap)
    return dev.results()


def check(pb, hap_ref_pos, mode=FIRST_MAX, hap_aligned=None, ops_cap=8, pairs=None, n_indels=None, use_on_hap=True, **kw):
    res = run(pb, hap_ref_pos, mode, hap_aligned, ops_cap, pairs=pairs, n_indels=n_indels, use_on_hap=use_on_hap, **kw)
    hap, none, pair = choose(pb, mode, res["ll"], res["onHap"] if use_on_hap else None, pairs, n_indels)
    got = {k: res["realign_" + k] for k in ("hap", "status", "n_ops", "ops", "ref_off")}
    assert np.array_equal(got["hap"], hap), "hap differs first at read %d" % int(np.argwhere(got["hap"] != hap)[0][0])
    # reads for which nothing is chosen: their code, no operation written
    off = hap < 0
    assert np.array_equal(got["status"][off], none[off]) and (got["n_ops"][off] == 0).all() and (got["ref_off"][off] == -1).all()
    assert (got["ops"][off] == FILL).all()
    # the chosen pairs: the host's CIGAR, and the very row of the per-pair launch
    want = host_rows(pb, pair, res["hpos"], hap_ref_pos, hap_aligned, res["status"], ops_cap)
    on = ~off
    cc.assert_equal({k: got[k][on] for k in want}, {k: want[k][on] for k in want})
    for k in ("status", "n_ops", "ops", "ref_off"):
        assert np.array_equal(got[k][on], res["cigar_" + k][pair[on]]), k
    return dict(got, pair=pair, none=none, res=res)


# ---------------------------------------------------------------- hand-made inputs
def shapes_batch(H, read_counts=(1, 63, 64, 65, 130), seed=0):
    """Windows of R = 1, 63, 64, 65 and 130 reads with H haplotypes each, reads of 1, 63, 64, 65, 130 and other lengths; empty windows (no
    read; with and without haplotypes) first, in the middle and last, and one window with reads and no haplotype."""
    rng = np.random.default_rng(seed)
    lens = [1, 63, 64, 65, 130]
    wins = [([], []), ([HAP_LEN] * H, [])]
    for i, R in enumerate(read_counts):
        wins.append(([HAP_LEN] * H, [lens[(i + k) % 5] if k < 5 else int(rng.integers(1, 131)) for k in range(R)]))
        if i == 1:
            wins += [([], []), ([], [20, 30, 40]), ([HAP_LEN] * H, [])]
    wins += [([HAP_LEN] * H, []), ([], [])]
    return cc.csr_batch(wins)


def made_hpos(pb, seed):
    """Per pair an alignment of its own (start, and sometimes a deletion or an insertion), so that a CIGAR names the pair it came from."""
    rng = np.random.default_rng(seed)
    hpos = np.zeros(pb.hpos_len, np.int16)
    for _p, _g, sl in cc.pair_hpos_slices(pb):
        L = sl.stop - sl.start
        start = int(rng.integers(-5, 120))
        v = np.arange(start, start + L)
        k = int(rng.integers(2, L - 3)) if L > 8 and rng.random() < 0.5 else -1
        ins = k >= 0 and rng.random() < 0.5
        if k >= 0 and not ins:
            v[k:] += int(rng.integers(1, 4))
        if ins:
            v[k + 1:] -= 1
        v = np.where(v < 0, capi.DD_HPOS_LO, np.where(v >= HAP_LEN, capi.DD_HPOS_RO, v))
        if ins and 0 <= v[k - 1]:
            v[k] = capi.DD_HPOS_INS_KEY0 - int(v[k - 1]) - 1
        hpos[sl] = v
    return hpos


def columns(pb):
    """(window, first pair of the read's column, stride R, H) per read."""
    a = pb.a
    for w in range(pb.n_windows):
        q0, R = int(a["win_read_off"][w]), int(a["win_read_off"][w + 1] - a["win_read_off"][w])
        H = int(a["win_hap_off"][w + 1] - a["win_hap_off"][w])
        for r in range(R):
            yield q0 + r, int(pb.win_pair_off[w]) + r, R, H


def first_max_likelihoods(pb, seed):
    """Random finite ll, then per read one of the patterns the rule must get right (in turn, over the reads of the batch)."""
    rng = np.random.default_rng(seed)
    ll = -rng.random(pb.n_pairs) * 50.0 - 1.0
    seen = set()
    for q, p0, R, H in columns(pb):
        if H == 0:
            continue
        col = ll[p0:p0 + H * R:R]                        # a view: writes land in ll
        top = float(col.max()) + 1.0
        kind = q % 14
        tie = {1: (0, 3), 2: (63, 64), 3: (64, 65)}.get(kind)
        if tie and tie[1] < H:
            col[tie[0]] = col[tie[1]] = top              # a tie: the first wins
        elif kind == 4:
            col[:] = -INF                                # nothing compares greater than -inf: haplotype 0
        elif kind == 5:
            col[:] = NAN
        elif kind == 6 and H > 1:
            col[0] = NAN                                 # NaN in front of the maximum
            col[H - 1] = top
        elif kind == 7 and H > 1:
            col[0] = top
            col[H - 1] = NAN                             # ... behind it
        elif kind == 8:
            col[int(np.argmax(col))] = NAN               # ... instead of it: the runner-up wins
        elif kind == 9:
            col[H // 2] = INF
            col[H - 1] = INF                             # +inf twice: the first
        elif kind == 10 and H > 2:
            col[:] = -INF
            col[H - 2] = -1e300                          # one finite value among -inf
        elif kind == 11:
            col[H - 1] = top                             # the last haplotype
        else:
            continue
        seen.add(kind)
    return ll, seen


@pytest.mark.parametrize("H", [1, 2, 8, 64, 65, 130])
def test_first_max_rule_on_hand_made_likelihoods(H):
    pb = shapes_batch(H, seed=H) if H < 64 else shapes_batch(H, read_counts=(1, 65, 130), seed=H)
    rng = np.random.default_rng(100 + H)
    ll, seen = first_max_likelihoods(pb, H)
    assert seen >= {4, 5, 8, 9, 11} and (H < 66 or seen >= {1, 2, 3, 6, 7, 10})
    on_hap = (rng.random(pb.n_reads) < 0.8).astype(np.uint8)
    status = rng.choice([0, 0, 0, 0, 0, 0, capi.DD_PAIR_NAN, capi.DD_PAIR_UNSUPPORTED], pb.n_pairs).astype(np.int32)
    hal = np.ones(pb.n_haps, np.uint8)
    hal[rng.random(pb.n_haps) < 0.1] = 0
    hrp = cc.batch_hap_ref_pos(pb, 7)
    hpos = made_hpos(pb, H)
    got = check(pb, hrp, FIRST_MAX, hal, ll=ll, on_hap=on_hap, hpos=hpos, status=status)
    st = got["status"]
    assert (st == capi.DD_REALIGN_OFF_HAP).sum() == int((on_hap[got["none"] != capi.DD_REALIGN_NO_HAPS] == 0).sum()) > 0
    assert (st == capi.DD_REALIGN_NO_HAPS).sum() == 3
    assert (st == capi.DD_CIGAR_OK).sum() > pb.n_reads // 3 and (st == capi.DD_CIGAR_NOT_COMPUTED).any()   # a chosen pair without a likelihood
    if H >= 8:
        assert (st == capi.DD_CIGAR_HAP_NOT_ALIGNED).any() and len(np.unique(got["hap"])) > min(H, 8) // 2
    # without onHap (NULL) every read with a haplotype gets one
    got = check(pb, hrp, FIRST_MAX, hal, ll=ll, hpos=hpos, status=status, use_on_hap=False)
    assert not (got["status"] == capi.DD_REALIGN_OFF_HAP).any() and (got["hap"] >= 0).sum() == pb.n_reads - 3


def pair_likelihoods(pb, pairs, seed):
    """ll whose (h1, h2) entries differ by 0, by just under / exactly / just over 1e-8 as fp64 computes the difference, in either
    direction, or hold NaN / -inf / +inf on either side or both (per read, in turn)."""
    rng = np.random.default_rng(seed)
    ll = -rng.random(pb.n_pairs) * 50.0 - 1.0
    below, above = np.nextafter(1e-8, 0.0), np.nextafter(1e-8, 1.0)
    kinds = [(0.0, 0.0), (below, 0.0), (1e-8, 0.0), (above, 0.0), (0.0, below), (0.0, 1e-8), (0.0, above), (-3.0, -3.0 + 1e-8), (-3.0 + 1e-8, -3.0),
             (NAN, -1.0), (-1.0, NAN), (NAN, NAN), (-INF, -1.0), (-1.0, -INF), (-INF, -INF), (INF, INF), (INF, -1.0), (-2.0, -1.0), (-1.0, -2.0)]
    a = pb.a
    for q, p0, R, H in columns(pb):
        w = int(np.searchsorted(a["win_read_off"], q, side="right") - 1)
        h1, h2 = int(pairs[2 * w]), int(pairs[2 * w + 1])
        if 0 <= h1 < H and 0 <= h2 < H and h1 != h2:
            ll[p0 + h1 * R], ll[p0 + h2 * R] = kinds[q % len(kinds)]
    return ll


@pytest.mark.parametrize("H", [1, 2, 8, 65])
def test_pair_rule_on_hand_made_likelihoods(H):
    pb = shapes_batch(H, read_counts=(1, 63, 64, 65, 130, 40, 40, 40, 40), seed=H)
    rng = np.random.default_rng(200 + H)
    W = pb.n_windows
    pairs = rng.integers(0, H, 2 * W).astype(np.int32)
    with_reads = [w for w in range(W) if pb.a["win_read_off"][w + 1] > pb.a["win_read_off"][w] and pb.a["win_hap_off"][w + 1] > pb.a["win_hap_off"][w]]
    assert len(with_reads) == 9
    if H > 1:
        pairs[2 * with_reads[0]:2 * with_reads[0] + 2] = (H - 1, 0)
        pairs[2 * with_reads[4]:2 * with_reads[4] + 2] = (0, H - 1)
    pairs[2 * with_reads[3]:2 * with_reads[3] + 2] = (H // 2, H // 2)             # h1 == h2
    for w, bad in zip(with_reads[5:], [(-1, 0), (0, -1), (H, 0), (0, H)]):        # outside [0, H): the whole window is refused
        pairs[2 * w:2 * w + 2] = bad
    n_indels = rng.integers(0, 3, pb.n_haps).astype(np.int32)                     # fewer on either side, and equal counts
    ll = pair_likelihoods(pb, pairs, H)
    on_hap = np.zeros(pb.n_reads, np.uint8)                                       # not consulted: every read gets a CIGAR
    hrp = cc.batch_hap_ref_pos(pb, 8)
    got = check(pb, hrp, PAIR, ll=ll, on_hap=on_hap, hpos=made_hpos(pb, 50 + H), pairs=pairs, n_indels=n_indels)
    st = got["status"]
    assert (st == capi.DD_REALIGN_BAD_PAIR).sum() == 4 * 40 and (st == capi.DD_REALIGN_NO_HAPS).sum() == 3
    assert not (st == capi.DD_REALIGN_OFF_HAP).any()
    if H > 1:                                                                      # the differences are what they were meant to be
        w0 = with_reads[4]
        p0, R = int(pb.win_pair_off[w0]), int(pb.a["win_read_off"][w0 + 1] - pb.a["win_read_off"][w0])
        with np.errstate(invalid="ignore"):
            d = np.abs(ll[p0:p0 + R] - ll[p0 + (H - 1) * R:p0 + H * R])
        assert (d == 0).any() and (d == 1e-8).any() and ((d < 1e-8) & (d > 0.9e-8)).any() and ((d > 1e-8) & (d < 1.1e-8)).any() and np.isnan(d).any()
        assert set(np.unique(got["hap"][got["hap"] >= 0])) >= {0, H - 1}


@pytest.mark.parametrize("ops_cap", [16, 2, 1])
def test_adversarial_alignments_as_chosen_pairs(ops_cap):
    """The alignments no traceback emits (every branch and every throw of the walk, events on bases 63 / 64 / 65), each as the chosen pair of
    its read: by the pooled rule over random likelihoods and by the diploid rule over the windows' two haplotypes."""
    pb, hpos, hrp = cc.adversarial_batch()
    rng = np.random.default_rng(ops_cap)
    ll = -rng.random(pb.n_pairs) * 9.0
    got = check(pb, hrp, FIRST_MAX, ops_cap=ops_cap, ll=ll, hpos=hpos, use_on_hap=False)
    assert set(np.unique(got["status"])) >= {capi.DD_CIGAR_ERROR2, capi.DD_CIGAR_ERROR3, capi.DD_CIGAR_ERROR4, capi.DD_CIGAR_IMPOSSIBLE}
    if ops_cap < 16:
        over = got["status"] == capi.DD_CIGAR_OVERFLOW
        assert over.sum() > 25 and (got["n_ops"][over] > ops_cap).all() and (got["ops"][over] != FILL).all()
    pairs = np.tile(np.array([1, 0], np.int32), pb.n_windows)
    got2 = check(pb, hrp, PAIR, ops_cap=ops_cap, ll=ll, hpos=hpos, pairs=pairs, n_indels=np.zeros(pb.n_haps, np.int32))
    assert np.array_equal(got2["hap"], got["hap"])                                # two haplotypes, no tie: the likelier one either way


# ---------------------------------------------------------------- behind the likelihood launches
def _long_window(rng, hap_len, L, R=6):
    hap = "".join(rng.choice(list("ACGT"), hap_len))
    hap2 = hap[:hap_len // 2] + "GT" + hap[hap_len // 2:]
    reads = []
    for _ in range(R):
        off = int(rng.integers(-L // 3, max(1, hap_len - L // 2)))
        src = hap2 if rng.random() < 0.5 else hap
        seq = "".join(src[i] if 0 <= i < len(src) else "A" for i in range(off, off + L))
        reads.append(ReadRec(seq, [0.999] * L, 0.9999, 1000 + off))
    return Window(1000, [hap, hap2], reads)


def _window_pairs(pb, seed):
    rng = np.random.default_rng(seed)
    nh = np.diff(pb.a["win_hap_off"])
    return np.stack([rng.integers(0, np.maximum(nh, 1)), rng.integers(0, np.maximum(nh, 1))], 1).astype(np.int32).reshape(-1)


def test_behind_the_main_launch_on_a_ragged_batch():
    """ll, onHap, status and hpos as dd_launch_device left them."""
    pb = synth.generate_ragged(14, seed=99, max_reads=120)
    hrp = cc.batch_hap_ref_pos(pb, 5)
    hal = np.ones(pb.n_haps, np.uint8)
    hal[::7] = 0
    got = check(pb, hrp, FIRST_MAX, hal, launch="main")
    assert (got["status"] == capi.DD_CIGAR_OK).sum() > pb.n_reads // 2 and len(np.unique(got["hap"])) > 2
    n_indels = np.random.default_rng(3).integers(0, 3, pb.n_haps).astype(np.int32)
    got = check(pb, hrp, PAIR, hal, launch="main", pairs=_window_pairs(pb, 4), n_indels=n_indels)
    assert (got["hap"] >= 0).all()


def test_behind_the_faster_and_the_long_window_launches():
    pb = synth.generate(4, H=4, R=40, L=100, hap_len=120, seed=8)
    got = check(pb, cc.batch_hap_ref_pos(pb, 2), FIRST_MAX, launch="faster")
    assert (got["status"] == capi.DD_CIGAR_OK).any()
    rng = np.random.default_rng(31)
    pbl = pack([_long_window(rng, 900, 150), _long_window(rng, 300, 1100, R=4), _long_window(rng, 200, 100)])
    hrpl = cc.batch_hap_ref_pos(pbl, 9)
    got = check(pbl, hrpl, FIRST_MAX, launch="main", long_windows=True)
    assert np.isin(got["status"], [capi.DD_CIGAR_OK, capi.DD_CIGAR_OVERFLOW, capi.DD_REALIGN_OFF_HAP]).all()
    got = check(pbl, hrpl, FIRST_MAX, launch="main", use_on_hap=False)           # without the option the long windows' pairs are not computed
    assert (got["status"] == capi.DD_CIGAR_NOT_COMPUTED).sum() == 6 + 4


def test_more_reads_than_the_grid_has_wavefront_slots():
    """The grid is persistent (2,048 workgroups x 4 wavefronts, 64 reads each): one full round and a partial one.  Three windows of one short
    haplotype and 36-bp reads; 97 distinct alignments in turn, so that the expectation is 97 host walks."""
    slots = 2048 * 4 * 64
    counts = [slots // 3 + 11, slots // 3 + 300, slots // 3 + 77]
    K, L = 97, 36
    pb = cc.csr_batch([([60], [L] * n) for n in counts])
    assert pb.n_reads > slots and pb.n_pairs == pb.n_reads
    rng = np.random.default_rng(12)
    hrp = cc.batch_hap_ref_pos(pb, 4, p_ins=0.0)                                  # (no inserted haplotype base: no walk here throws)
    pat = np.zeros((K, L), np.int16)
    for k in range(K):
        v = np.arange(L) + int(rng.integers(-4, 30))
        if k % 3 == 1:
            v[int(rng.integers(3, L - 3)):] += int(rng.integers(1, 4))
        pat[k] = np.where(v < 0, capi.DD_HPOS_LO, np.where(v >= 60, capi.DD_HPOS_RO, v))
    which = np.arange(pb.n_reads) % K
    hpos = pat[which].reshape(-1)                                                 # H = 1: the pair's alignment is the read's
    assert len(hpos) == pb.hpos_len
    on_hap = (rng.random(pb.n_reads) < 0.9).astype(np.uint8)
    res = run(pb, hrp, FIRST_MAX, ll=-rng.random(pb.n_pairs), on_hap=on_hap, hpos=hpos)
    hso = pb.a["hap_seq_off"]
    assert (np.diff(hso) == 60).all()
    on = on_hap != 0
    assert np.array_equal(res["realign_hap"], np.where(on, 0, -1))
    assert (res["realign_status"][~on] == capi.DD_REALIGN_OFF_HAP).all() and (res["realign_ops"][~on] == FILL).all()
    assert (res["realign_n_ops"][~on] == 0).all() and (res["realign_ref_off"][~on] == -1).all()
    for k in ("status", "n_ops", "ops", "ref_off"):                               # the per-pair launch's rows, read for read
        assert np.array_equal(res["realign_" + k][on], res["cigar_" + k][on]), k
    win = np.searchsorted(pb.a["win_read_off"], np.arange(pb.n_reads), side="right") - 1
    for w in range(3):                                                            # the host's walk: per window (its haplotype's map) the 97 alignments
        cig = [cc.host_cigar(hrp[hso[w]:hso[w + 1]], pat[k]) for k in range(K)]
        assert all(not isinstance(c, int) and len(c[0]) <= 8 for c in cig)
        n_ops = np.array([len(c[0]) for c in cig], np.int32)
        ref_off = np.array([c[1] for c in cig], np.int32)
        first = np.array([(c[0][0][1] << 4) | c[0][0][0] for c in cig], np.uint32)
        m = on & (win == w)
        assert m.sum() > slots // 4
        assert (res["realign_status"][m] == capi.DD_CIGAR_OK).all()
        assert np.array_equal(res["realign_n_ops"][m], n_ops[which[m]]) and np.array_equal(res["realign_ref_off"][m], ref_off[which[m]])
        assert np.array_equal(res["realign_ops"][m, 0], first[which[m]])


# ---------------------------------------------------------------- the host-pointer entry
def host_entry(lib, pb, hrp, hal, mode=FIRST_MAX, pairs=None, n_indels=None, ops_cap=8, options=0, with_hpos=False, with_on_hap=True, result=None):
    p = capi.params_cli_defaults()
    arrs, res = result or alloc_result(pb)
    if not with_hpos:
        res.hpos = None
        arrs["hpos"][:] = -12345
    if not with_on_hap:
        res.onHap = None
    out, rl = capi.realign_arrays(pb.n_reads, ops_cap)
    for v in out.values():
        v[...] = FILL
    b = pb.ctypes_batch()
    rc = lib.dd_compute_likelihoods_realign(C.byref(p), C.byref(b), C.byref(res), mode, None if pairs is None else pairs.ctypes.data_as(capi.c_i32p),
                                            None if n_indels is None else n_indels.ctypes.data_as(capi.c_i32p), hrp.ctypes.data_as(capi.c_i32p),
                                            None if hal is None else hal.ctypes.data_as(capi.c_u8p), C.byref(rl), ops_cap, 0, options)
    assert rc == 0, capi.last_error()
    return out, arrs


def assert_same_reads(out, got):
    """The host-pointer entry against the device-pointer path (checked above against the host): a read's operation slots beyond its count
    come back as zero on this path, and a read for which nothing is chosen keeps whatever the caller had there."""
    for k in ("hap", "status", "n_ops", "ref_off"):
        assert np.array_equal(out[k], got[k]), k
    cap = out["ops"].shape[1]
    written = np.arange(cap)[None, :] < np.minimum(got["n_ops"], cap)[:, None]
    finished = np.isin(got["status"], [capi.DD_CIGAR_OK, capi.DD_CIGAR_OVERFLOW])[:, None]
    assert np.array_equal(out["ops"][written], got["ops"][written]) and (out["ops"][~written & finished] == 0).all()


def test_host_entry_keeps_everything_else_on_the_device(lib):
    """dd_compute_likelihoods_realign with and without r->hpos, both rules, with DD_OPT_LONG_WINDOWS: the device-pointer path's reads, the other
    outputs of dd_compute_likelihoods, and no alignment copied back unless asked for."""
    pb = synth.generate(5, H=5, R=60, L=100, hap_len=130, seed=1334, vary_read_len=True, mixed_quals=True)
    hrp = cc.batch_hap_ref_pos(pb, 77)
    hal = np.ones(pb.n_haps, np.uint8)
    hal[3] = 0
    got = check(pb, hrp, FIRST_MAX, hal, launch="main")
    out, arrs = host_entry(lib, pb, hrp, hal)
    assert_same_reads(out, got)
    assert (arrs["hpos"] == -12345).all()
    plain, _res = alloc_result(pb)
    p = capi.params_cli_defaults()
    b = pb.ctypes_batch()
    assert lib.dd_compute_likelihoods(C.byref(p), C.byref(b), C.byref(_res), 0) == 0
    for k in plain:
        if k != "hpos":
            assert np.array_equal(plain[k], arrs[k]), k
    out2, arrs2 = host_entry(lib, pb, hrp, hal, with_hpos=True)                  # asking for the alignments as well changes nothing else
    assert_same_reads(out2, got)
    assert np.array_equal(arrs2["hpos"], plain["hpos"])
    got_all = check(pb, hrp, FIRST_MAX, hal, launch="main", use_on_hap=False)    # a caller that does not ask for onHap: the rule without it
    out3, _ = host_entry(lib, pb, hrp, hal, with_on_hap=False)
    assert_same_reads(out3, got_all)
    pairs, n_indels = _window_pairs(pb, 6), np.random.default_rng(7).integers(0, 3, pb.n_haps).astype(np.int32)
    got_pair = check(pb, hrp, PAIR, hal, launch="main", pairs=pairs, n_indels=n_indels)
    out4, _ = host_entry(lib, pb, hrp, hal, PAIR, pairs, n_indels, ops_cap=3)
    got_pair3 = check(pb, hrp, PAIR, hal, ops_cap=3, launch="main", pairs=pairs, n_indels=n_indels)
    assert np.array_equal(got_pair["hap"], got_pair3["hap"])
    assert_same_reads(out4, got_pair3)
    # with the long-window option, and a window without haplotypes between the others
    rng = np.random.default_rng(31)
    pbl = pack([_long_window(rng, 900, 150), Window(1000, [], [ReadRec("ACGT" * 9, [0.999] * 36, 0.9999, 1000)] * 2), _long_window(rng, 200, 100)])
    hrpl = cc.batch_hap_ref_pos(pbl, 9)
    gotl = check(pbl, hrpl, FIRST_MAX, launch="main", long_windows=True)
    assert (gotl["status"] == capi.DD_REALIGN_NO_HAPS).sum() == 2
    outl, _ = host_entry(lib, pbl, hrpl, None, options=capi.DD_OPT_LONG_WINDOWS)
    assert_same_reads(outl, gotl)
    outn, _ = host_entry(lib, pbl, hrpl, None, with_on_hap=False)                # without it the long window's reads name pairs that were not computed
    assert (outn["status"][:6] == capi.DD_CIGAR_NOT_COMPUTED).all() and (outn["status"][6:8] == capi.DD_REALIGN_NO_HAPS).all()


def test_host_entry_with_page_locked_results(lib):
    """dd_compute_likelihoods_realign with every dd_result array in page-locked memory: the realign launch reads hpos, ll and onHap on the
    device, so these three — which a plain call lets the kernels write in place — are staged in HBM and copied back; every byte equals the
    pageable call's."""
    pb = synth.generate(5, H=5, R=60, L=100, hap_len=130, seed=1334, vary_read_len=True, mixed_quals=True)
    hrp = cc.batch_hap_ref_pos(pb, 77)
    hal = np.ones(pb.n_haps, np.uint8)
    hal[3] = 0
    want, pageable = host_entry(lib, pb, hrp, hal, with_hpos=True)
    assert lib.dd_last_direct_outputs() == 0
    got, pinned, direct, plain = with_page_locked_results(lib, pb, lambda result: host_entry(lib, pb, hrp, hal, with_hpos=True, result=result))
    assert direct == plain - 3
    assert_same_bytes(pb, pageable, pinned)
    for k in want:
        assert np.array_equal(want[k], got[k]), k


def test_host_entry_in_window_blocks(lib):
    """A batch of more than a million pairs runs as window blocks on two streams: every block's reads arrive, equal to the device-pointer path's."""
    small = synth.generate(8, H=8, R=200, L=60, hap_len=100, seed=5)
    pb = synth.tile(small, 90)
    assert pb.n_pairs > 1100000
    hrp = cc.batch_hap_ref_pos(pb, 1)
    res = run(pb, hrp, FIRST_MAX, ops_cap=4, launch="main")
    got = {k: res["realign_" + k] for k in ("hap", "status", "n_ops", "ops", "ref_off")}
    assert (got["status"] == capi.DD_CIGAR_OK).any() and (got["status"] == capi.DD_REALIGN_OFF_HAP).sum() < pb.n_reads // 2
    out, _ = host_entry(lib, pb, hrp, None, ops_cap=4)
    assert_same_reads(out, got)
    n1 = int(small.a["win_read_off"][1])                                          # the first window against the rules and the host walk
    first = small.slice_windows(0, 1)
    hap, none, pair = choose(first, FIRST_MAX, res["ll"][:int(small.win_pair_off[1])], res["onHap"][:n1])
    assert np.array_equal(got["hap"][:n1], hap)
    want = host_rows(first, pair, res["hpos"][:int(small.win_hpos_off[1])], hrp[:int(small.a["hap_seq_off"][8])], None, res["status"][:int(small.win_pair_off[1])], 4)
    on = hap >= 0
    for k in ("status", "n_ops", "ref_off"):
        assert np.array_equal(got[k][:n1][on], want[k][on]), k
