"""Candidate discovery on the device.  The indel events of dd_align_events_kernel (csrc/align_events_kernel.hip) against the
restatement's column scan of the two gapped rows (tests/_candidates_oracle.py; tests/test_candidates_cpu.py pins that scan's rules against
the rows of the reference's SeqAn), field for field; then the tool host/dindel_candidates end to end against the restatement, byte for
byte."""
import json
import os
import random

import numpy as np
import pytest

from dindel_tgi_amd import capi, hapalign
from tests import _candidates_cases as cases, _candidates_oracle as cand, _hapalign_oracle as orc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = -21846                                   # 0xAAAA: what the event records hold where the kernel must not write


def as_tuples(events, n):
    return [tuple(int(v) for v in row) for row in events[:n]]


def check_guards():
    assert hapalign.last_launch()["guard_trips"] == 0 and hapalign.events_last_launch()["guard_trips"] == 0


# ---- kernel = restatement -------------------------------------------------------------------------------------------------------------------

def test_all_seqan_fixtures_in_one_launch():
    fx = json.load(open(os.path.join(HERE, "golden", "hapalign_seqan.json")))
    refs = [c["ref"].encode("latin-1") for c in fx]
    haps = [c["hap"].encode("latin-1") for c in fx]
    want = [cand.events_from_rows(c["row0"], c["row1"]) for c in fx]
    cap = max(len(w) for w in want)
    got = hapalign.align_events(refs, haps, list(range(len(fx))), events_cap=cap)
    check_guards()
    assert hapalign.events_last_launch()["pairs"] == len(fx)
    assert np.all(got["status"] == 0) and got["score"].tolist() == [c["score"] for c in fx]
    for i, w in enumerate(want):
        assert got["n_events"][i] == len(w) and as_tuples(got["events"][i], len(w)) == w, (i, fx[i], w)
        assert np.all(got["events"][i, len(w):] == 0), i


def slice_of(segs):
    """(slice, reference length) of an alignment given as [(op, n)]: M paired, I haplotype bases facing a gap, D deleted reference bases"""
    pos, r = [], 0
    for op, n in segs:
        if op == "M":
            pos += list(range(r, r + n))
        elif op == "I":
            pos += [-1 - r] * n
        r += n if op in "MD" else 0
    return pos, r


def built_cases():
    out = [[("M", 1)], [("I", 1)], [("D", 3), ("M", 1)], [("M", 1), ("D", 2)],
           [("I", 2), ("M", 5)],                              # a leading insertion
           [("D", 2), ("M", 5)], [("I", 2), ("D", 2), ("M", 5)],   # a deletion in front of the first paired base
           [("M", 5), ("I", 2)],                              # a trailing insertion at the reference's end
           [("M", 5), ("D", 2)],                              # a trailing deletion
           [("M", 5), ("I", 2), ("D", 2)], [("M", 5), ("D", 2), ("I", 2)],
           # both orders of a block substitution, twice each in one pair
           [("M", 5), ("D", 3), ("I", 2), ("M", 5), ("I", 2), ("D", 3), ("M", 5), ("D", 2), ("I", 1), ("M", 4), ("I", 3), ("D", 1), ("M", 3)]]
    for L in (1, 63, 64, 65, 127, 128, 129, 200):
        out.append([("M", L)])
        for c in (64, 128):
            if c > L:
                continue
            for start, n in ((c, 3), (c - 3, 3), (c - 2, 4), (c - 1, 1), (c - 64 + 1, 63), (c - 64 + 1, 64)):
                if start < 1 or start + n > L:
                    continue
                rest = L - start - n
                out.append([("M", start), ("I", n)] + ([("M", rest)] if rest else [("D", 1)]))         # an insertion on / up to / across the boundary
                if rest:
                    out.append([("M", start), ("D", n), ("M", L - start)])                                # a deletion in front of base `start`
                    out.append([("M", start), ("D", 2), ("I", n), ("M", rest)])
                    out.append([("M", start), ("I", n), ("D", 2), ("M", rest)])
        if L == 200:
            out.append([("M", 60), ("I", 70), ("M", 70)])                                                 # a run over a whole chunk
            out.append([("M", 1), ("I", 198), ("M", 1)])
            out.append([("I", 70), ("M", 130)])                                                            # LO over a boundary
            out.append([("M", 100), ("I", 100)])                                                           # RO over a boundary
    return out


def run_built(segs_list, cap, stream=None):
    """events of hand-built slices: a DeviceAlign over placeholder sequences of the right lengths is launched (the event launch runs
    behind an alignment launch), its slices are replaced, then the events are extracted"""
    import torch
    slices = [slice_of(s) for s in segs_list]
    refs = [b"A" * max(r, 1) for _, r in slices]
    haps = [b"C" * len(p) for p, _ in slices]
    dev = hapalign.DeviceAlign(refs, haps, list(range(len(refs))), "cuda:0")
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        dev.launch(stream)
        dev.ref_pos.copy_(torch.tensor([v for p, _ in slices for v in p], dtype=torch.int16), non_blocking=False)
        dev.status.zero_()
        dev.launch_events(cap, stream, fill=SENTINEL)
    got = dev.event_results()
    check_guards()
    want = []
    for (p, r), ref, hap in zip(slices, refs, haps):
        row0, row1 = hapalign.gapped_rows(ref[:r] if r else b"", hap, p) if r else ("-" * len(p), "C" * len(p))
        want.append(cand.events_from_rows(row0, row1))
    return got, want


def test_built_slices_at_the_chunk_boundaries():
    segs = built_cases()
    assert len(segs) > 80
    got, want = run_built(segs, 8)
    assert max(len(w) for w in want) == 8 and sum(1 for w in want if not w) >= 12
    for i, w in enumerate(want):
        assert got["n_events"][i] == len(w) and as_tuples(got["events"][i], len(w)) == w, (segs[i], as_tuples(got["events"][i], 8), w)
        assert np.all(got["events"][i, len(w):] == SENTINEL), segs[i]


@pytest.mark.parametrize("cap", [1, 2])
def test_more_events_than_the_cap(cap):
    """pairs with three events between pairs with none: the true count, the first `cap` records, and nothing behind them — the rows of
    the pairs without events lie right behind and stay untouched"""
    three = [[("M", 4), ("I", 2), ("M", 60), ("D", 3), ("M", 10), ("I", 1), ("M", 5)], [("M", 62), ("I", 5), ("D", 2), ("M", 70), ("D", 1), ("M", 3)]]
    segs = [three[0], [("M", 30)], three[1], [("I", 3), ("M", 9)], three[0], [("M", 70), ("D", 4)]]
    got, want = run_built(segs, cap)
    assert [len(w) for w in want] == [3, 0, 3, 0, 3, 0]
    for i, w in enumerate(want):
        kept = min(len(w), cap)
        assert got["n_events"][i] == len(w) and as_tuples(got["events"][i], kept) == w[:kept], i
        assert np.all(got["events"][i, kept:] == SENTINEL), i


def test_statuses_between_good_pairs_and_an_empty_batch():
    rng = random.Random(31)
    good = bytes(rng.choice(b"ACGT") for _ in range(80))
    too_long = bytes(rng.choice(b"ACGT") for _ in range(capi.DD_LONG_MAX_HAP_LEN + 1))
    refs = [good, b"", too_long]
    haps = [good[:30] + b"TT" + good[30:], b"", good[:50] + good[53:], good, too_long[:300], good[:20] + good[22:]]
    pair_ref = [0, 0, 0, 1, 2, 0]
    got = hapalign.align_events(refs, haps, pair_ref, events_cap=4)
    check_guards()
    assert got["status"].tolist() == [0, capi.DD_ALIGN_EMPTY, 0, capi.DD_ALIGN_EMPTY, capi.DD_ALIGN_TOO_LONG, 0]
    for i in range(6):
        if got["status"][i]:
            assert got["n_events"][i] == 0 and got["score"][i] == 0 and np.all(got["events"][i] == 0), i
        else:
            _, row0, row1, _ = orc.align(refs[pair_ref[i]], haps[i])
            w = cand.events_from_rows(row0, row1)
            assert len(w) == 1 and got["n_events"][i] == 1 and as_tuples(got["events"][i], 1) == w, i
    none = hapalign.align_events([], [], [], events_cap=4)
    assert len(none["n_events"]) == 0 and len(none["score"]) == 0


@pytest.mark.parametrize("n_pairs", [5000, 20000])
def test_many_pairs_on_the_persistent_grid(n_pairs):
    rng = random.Random(32)
    distinct = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(18, 24))) for _ in range(100)]
    variants = {}
    for r in distinct:
        p = rng.randrange(4, 12)
        variants[r] = [r, r[:p] + b"G" + r[p:], r[:p] + r[p + 2:], r[:p] + b"TT" + r[p + 3:]]
    want = {(r, h): cand.events_from_rows(*orc.align(r, h)[1:3]) for r in distinct for h in variants[r]}
    refs = [distinct[i % 100] for i in range(1000)]
    pair_ref = [i % 1000 for i in range(n_pairs)]
    haps = [variants[refs[r]][(i // 1000) % 4] for i, r in enumerate(pair_ref)]
    got = hapalign.align_events(refs, haps, pair_ref, events_cap=3)
    log = hapalign.events_last_launch()
    assert log["pairs"] == n_pairs and log["guard_trips"] == 0 and hapalign.last_launch()["guard_trips"] == 0, log
    assert 1 <= log["max_draws"] <= n_pairs and (n_pairs <= 4 * log["grid"] or log["max_draws"] >= 2), log
    assert np.all(got["status"] == 0)
    for i in range(n_pairs):
        w = want[(refs[pair_ref[i]], haps[i])]
        assert got["n_events"][i] == len(w) and as_tuples(got["events"][i], min(len(w), 3)) == w[:3], i


def test_device_entry_on_a_stream_and_null_ref_pos():
    import torch
    rng = random.Random(33)
    refs = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(150, 210))) for _ in range(30)]
    pair_ref = [i % 30 for i in range(240)]
    haps = []
    for r in pair_ref:
        s, p, q = refs[r], rng.randrange(10, 60), rng.randrange(80, 140)
        haps.append(s[:p] + bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 5))) + s[p:q] + s[q + rng.randint(1, 4):])
    without = hapalign.align_events(refs, haps, pair_ref, events_cap=4)
    with_slice = hapalign.align_events(refs, haps, pair_ref, events_cap=4, with_ref_pos=True)
    check_guards()
    for k in ("score", "status", "n_events", "events"):
        assert np.array_equal(without[k], with_slice[k]), k
    plain = hapalign.align_haplotypes(refs, haps, pair_ref)
    assert np.array_equal(with_slice["ref_pos"], plain["ref_pos"])
    off = plain["hap_off"]
    for i in range(len(haps)):
        w = cand.events_from_rows(*hapalign.gapped_rows(refs[pair_ref[i]], haps[i], plain["ref_pos"][off[i]:off[i + 1]]))
        assert without["n_events"][i] == len(w) and as_tuples(without["events"][i], min(len(w), 4)) == w[:4], i
    dev = hapalign.DeviceAlign(refs, haps, pair_ref, "cuda:0")
    stream = torch.cuda.Stream(device="cuda:0")
    for _ in range(2):                                  # the second round finds the first one's counters in the workspace header
        dev.launch(stream)
        dev.launch_events(4, stream, fill=0)
        got = dev.event_results()
        check_guards()
        assert np.array_equal(got["n_events"], without["n_events"]) and np.array_equal(got["events"], without["events"])


# ---- the tool ---------------------------------------------------------------------------------------------------------------------------

def test_align_cigar_end_to_end(tmp_path):
    """about 300 candidates in and around planted repeats: tool = restatement byte for byte, --hostConvert = default"""
    ref, cands = cases.repeat_reference()
    assert 250 <= len(cands) <= 400 and {33, 34} <= {abs(c[1]) for c in cands}
    fasta = str(tmp_path / "r.fa")
    cases.write_fasta(fasta, [("chr9", ref)])
    text = cases.candidate_file_text("chr9", cands, ref)
    vf = tmp_path / "in.txt"
    vf.write_text(text)
    want = cand.realign_file(text, False, {"chr9": ref})
    collisions = len(cands) - sum(len(l.split(" #")[0].split(" ")) - 2 for l in want.split("\n")[:-1])
    assert collisions > 50                              # several candidates land on one canonical variant
    outs = []
    for extra in ([], ["--hostConvert"], ["--eventsCap", "1", "--batchCandidates", "50"]):
        out = str(tmp_path / ("o%d" % len(outs)))
        rc, so, se = cases.run_tool(["--analysis", "realignCandidates", "--varFile", vf, "--ref", fasta, "--outputFile", out, "--quiet"] + extra)
        assert rc == 0, (so, se)
        outs.append(open(out + ".variants.txt").read())
    assert outs[0] == want and outs[1] == outs[0] and outs[2] == outs[0]


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    return cases.bam_sample(tmp_path_factory.mktemp("gcand"))


def test_whole_file_run(sample, tmp_path):
    want_v, want_l = cand.whole_file(sample["header"], sample["names"], sample["records"], sample["targets"])
    for k, extra in enumerate(([], ["--hostConvert"])):
        out = str(tmp_path / ("w%d" % k))
        rc, so, se = cases.run_tool(["--analysis", "getCIGARindels", "--bamFile", sample["bam"], "--ref", sample["fasta"], "--outputFile", out, "--quiet"] + extra)
        assert rc == 0, (so, se)
        assert open(out + ".variants.txt").read() == want_v and open(out + ".libraries.txt").read() == want_l


def test_region_run_over_two_files_and_realign_in_both_conventions(sample, tmp_path):
    from tests import _bamwriter
    second = cases.bam_sample(tmp_path, name="second", seed=12, n_reads=120)
    lst = tmp_path / "bams.txt"
    lst.write_text(sample["bam"] + "\n" + second["bam"] + "\n")
    out = str(tmp_path / "region.txt")
    rc, so, se = cases.run_tool(["--analysis", "getCIGARindels", "--bamFiles", lst, "--tid", "chrB", "--region", "100-1200", "--ref", sample["fasta"],
                                 "--outputFile", out, "--quiet"])
    assert rc == 0, (so, se)
    table = cand.Table()
    for s in (sample, second):
        for tid, r in s["records"]:
            if tid == 1 and r["pos"] < 1200 and r["pos"] + _bamwriter.ref_len(_bamwriter.parse_cigar(r["cigar"])) > 100:
                for c in cand.cigar_indels(r["pos"], r["cigar"], r["seq"]):
                    table.add(*c)
    region = cand.output_indels("chrB", table, sample["targets"]["chrB"])
    assert open(out).read() == region and region.count("\n") >= 5
    # the region's own output as a candidate file, zero-based; and the same candidates written one-based
    for one_based in (False, True):
        text = "".join("%s %d %s\n" % (l.split(" ")[0], int(l.split(" ")[1]) + one_based, " ".join(l.split(" ")[2:])) for l in region.split("\n")[:-1])
        vf = tmp_path / ("v%d.txt" % one_based)
        vf.write_text(text)
        o = str(tmp_path / ("re%d" % one_based))
        rc, so, se = cases.run_tool(["--analysis", "realignCandidates", "--varFile", vf, "--ref", sample["fasta"], "--outputFile", o, "--quiet"] +
                                    (["--varFileIsOneBased"] if one_based else []))
        assert rc == 0, (so, se)
        assert open(o + ".variants.txt").read() == cand.realign_file(text, one_based, sample["targets"])


def test_driver_accepts_the_library_file(sample, tmp_path, scene):
    out = str(tmp_path / "lib")
    rc, so, se = cases.run_tool(["--analysis", "getCIGARindels", "--bamFile", sample["bam"], "--ref", sample["fasta"], "--outputFile", out, "--quiet"])
    assert rc == 0, (so, se)
    _path, rows = run_driver(scene, "candlib", "--libFile", out + ".libraries.txt")
    assert len(rows) > 4 and any(r["msg"] == "ok" for r in rows)


from tests.test_n2_driver_gpu import run_driver, scene  # noqa: E402,F401  (the driver's sample and the way to run it)
