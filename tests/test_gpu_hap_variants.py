"""dd_hap_variants_kernel (csrc/hap_variants_kernel.hip) against its host twin hapVariantsHost (host/align_haplotypes.cpp, reached through
ddh_hap_variants_json), word for word: summaries and records.  tests/test_hap_variants_cpu.py pins the twin against the string walk of
convertHaplotypeAlignment.  The draw guard is 0 in every launch."""
import numpy as np
import pytest

from dindel_tgi_amd import capi, hapalign
from tests import _hap_variant_cases as hv

pytestmark = pytest.mark.gpu
SENTINEL = -21846                                   # 0xAAAA: what the records hold where the kernel must not write


def check_guards():
    assert hapalign.last_launch()["guard_trips"] == 0 and hapalign.variants_last_launch()["guard_trips"] == 0


def twin(cases, cap):
    """hapVariantsHost per pair -> (summary [n, 4], variants [n, cap, 8]); cases that share a reference go through one call"""
    n = len(cases)
    summary, variants = np.zeros((n, 4), np.int32), np.zeros((n, cap, 8), np.int16)
    by_ref = {}
    for i, (ref, _, _) in enumerate(cases):
        by_ref.setdefault(ref, []).append(i)
    for ref, idx in by_ref.items():
        for k in range(0, len(idx), 128):
            part = idx[k:k + 128]
            s, v, out = hv.twin_window(ref, [cases[i][1] for i in part], [cases[i][2] for i in part], cap)
            assert "throw" not in out, out
            summary[part], variants[part] = s, v
    return summary, variants


def run_device(cases, cap, stream=None, status=None, relaunch=False):
    """a DeviceAlign over the cases' sequences is launched (the variants launch runs behind an alignment launch), its slices are replaced
    by the cases' own, then the variants are extracted into tensors preset to SENTINEL"""
    import torch
    refs = [c[0] for c in cases]
    haps = [c[1] for c in cases]
    dev = hapalign.DeviceAlign(refs, haps, list(range(len(cases))), "cuda:0")
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        dev.launch(stream)
        dev.ref_pos.copy_(torch.tensor([v for c in cases for v in c[2]], dtype=torch.int16), non_blocking=False)
        dev.status.copy_(torch.tensor(status if status is not None else [0] * len(cases), dtype=torch.int32), non_blocking=False)
        dev.launch_variants(cap, stream, fill=SENTINEL)
        if relaunch:
            first = {k: v.clone() for k, v in (("summary", dev.summary), ("variants", dev.variants))}
            dev.launch_variants(cap, stream, fill=None)                 # a second launch into the same tensors
    got = dev.variant_results()
    check_guards()
    assert hapalign.variants_last_launch()["pairs"] == len(cases)
    if relaunch:
        assert np.array_equal(first["summary"].cpu().numpy(), got["summary"]) and np.array_equal(first["variants"].cpu().numpy(), got["variants"])
    return got


def compare(cases, got, cap):
    want_s, want_v = twin(cases, cap)
    for i in range(len(cases)):
        assert got["summary"][i].tolist() == want_s[i].tolist(), (i, cases[i][:2], got["summary"][i], want_s[i])
        kept = min(int(want_s[i][0]), cap)
        assert got["variants"][i, :kept].tolist() == want_v[i, :kept].tolist(), (i, cases[i][:2], got["variants"][i, :kept], want_v[i, :kept])
        assert np.all(got["variants"][i, kept:] == SENTINEL), (i, cases[i][:2])
    return want_s


def test_the_cpu_files_cases_in_one_launch():
    cases = hv.all_cases()
    got = run_device(cases, hv.CAP)
    want = compare(cases, got, hv.CAP)
    assert (want[:, 3] & capi.DD_HAP_VARIANTS_HOST).astype(bool).sum() >= 3 and want[:, 0].max() <= hv.CAP


def from_rows(row0, row1):
    return row0.replace("-", "").encode(), row1.replace("-", "").encode(), hv.ref_pos_of_rows(row0, row1)


def shape_cases():
    rng = np.random.default_rng(8)
    out = []
    for L in (1, 63, 64, 65, 127, 128, 129, 200):
        ref = "".join(rng.choice(list("ACGT"), L))
        out.append(from_rows(ref, ref))
        if L > 64:
            # a SNP at lane 0 of the second chunk, and a deletion in front of it (the predecessor is carried)
            alt = "ACGT"[("ACGT".index(ref[64]) + 1) % 4]
            out.append(from_rows(ref, ref[:64] + alt + ref[65:]))
            out.append(from_rows(ref[:64] + "GT" + ref[64:], ref[:64] + "--" + alt + ref[65:]))
            out.append(from_rows(ref[:64] + "G" + ref[64:], ref[:64] + "-" + ref[64:]))
        if L >= 127:
            for start, n in ((62, 4), (63, 1), (63, 2), (62, 2), (1, 63), (1, 64), (64, 3), (61, 3)):      # insertion runs on / across the chunk end
                out.append(from_rows(ref[:start] + "-" * n + ref[start:], ref[:start] + "".join(rng.choice(list("ACGT"), n)) + ref[start:]))
                out.append(from_rows(ref[:start] + "-" * n + "CA" + ref[start:], ref[:start] + "T" * n + "--" + ref[start:]))    # then a deletion at the same key
    ref = "".join(rng.choice(list("ACGT"), 200))
    out.append(from_rows(ref[:60] + "-" * 140 + ref[60:], ref[:60] + "".join(rng.choice(list("ACGT"), 140)) + ref[60:]))     # a run over three chunks
    out.append(from_rows("-" * 70 + ref, "T" * 70 + ref))                                                    # LO over a chunk end
    out.append(from_rows(ref + "-" * 70, ref + "T" * 70))                                                    # RO over a chunk end
    out.append(from_rows(ref[:64] + "-" * 64 + ref[64:], ref[:64] + "G" * 64 + ref[64:]))                    # exactly the second chunk
    # flank runs that cross one and two chunk ends of the search, in each direction: a deletion and an insertion inside a homopolymer and
    # inside a 2-mer repeat, run lengths 70 / 79 and 140 / 159 around the variant
    for n, sh in ((150, 71), (300, 141)):
        homo = "C" + "A" * n + "G"
        out.append(from_rows(homo, homo[:sh] + "-" + homo[sh + 1:]))
        out.append(from_rows(homo[:sh] + "-" + homo[sh:], homo[:sh] + "A" + homo[sh:]))
        rep = "C" + "AG" * (n // 2) + "T"
        out.append(from_rows(rep, rep[:sh] + "--" + rep[sh + 2:]))
        out.append(from_rows(rep[:sh] + "--" + rep[sh:], rep[:sh] + rep[sh:sh + 2] + rep[sh:]))
        out.append(from_rows("A" * n, "A" * sh + "-" + "A" * (n - sh - 1)))                                 # runs that reach both ends
    return out


def test_shapes_where_the_mapping_can_go_wrong():
    cases = shape_cases()
    assert len(cases) > 70
    got = run_device(cases, 8)
    want = compare(cases, got, 8)
    assert want[:, 0].max() <= 8 and (want[:, 0] == 0).sum() >= 8


@pytest.mark.parametrize("cap", [1, 4])
def test_exactly_cap_records_and_one_more(cap):
    """pairs with cap, cap + 1 and no records side by side: the true count, the first cap records, the sentinels behind every slice"""
    rng = np.random.default_rng(cap)
    ref = "".join(rng.choice(list("ACGT"), 90))

    def snps(k):
        h = list(ref)
        for j in range(k):
            at = 5 + 17 * j
            h[at] = "ACGT"[("ACGT".index(h[at]) + 1) % 4]
        return from_rows(ref, "".join(h))
    cases = [snps(cap), snps(0), snps(cap + 1), snps(0), snps(cap), snps(cap + 1)]
    got = run_device(cases, cap)
    want = compare(cases, got, cap)
    assert want[:, 0].tolist() == [cap, 0, cap + 1, 0, cap, cap + 1]


def test_pairs_that_were_not_aligned_between_good_ones():
    rng = np.random.default_rng(2)
    ref = "".join(rng.choice(list("ACGT"), 80))
    one = from_rows(ref[:40] + "--" + ref[40:], ref[:40] + "TT" + ref[40:])
    cases = [one] * 7
    status = [0, capi.DD_ALIGN_EMPTY, 0, capi.DD_ALIGN_TOO_LONG, capi.DD_ALIGN_BAD_REF, 0, capi.DD_ALIGN_EMPTY]
    got = run_device(cases, 4, status=status)
    want_s, want_v = twin([one], 4)
    for i, st in enumerate(status):
        if st:
            assert got["summary"][i].tolist() == [0, 0, 0, 0] and np.all(got["variants"][i] == SENTINEL), i
        else:
            assert got["summary"][i].tolist() == want_s[0].tolist() and got["variants"][i, :1].tolist() == want_v[0, :1].tolist(), i
            assert np.all(got["variants"][i, 1:] == SENTINEL)


def test_an_empty_batch():
    got = hapalign.align_variants([], [], [], cap=4)
    assert len(got["status"]) == 0 and len(got["summary"]) == 0
    assert capi.load().dd_hap_variants_device(None, None, None, None, 4, None) == capi.DD_ERR_INVALID


def test_more_pairs_than_the_grid_holds_wavefronts():
    """20,000 pairs of 8 ... 16 bases: the persistent grid is 2,048 workgroups of 4 wavefronts, so wavefronts draw several pairs each"""
    rng = np.random.default_rng(12)
    cases = []
    for _ in range(200):
        L = int(rng.integers(8, 17))
        ref = "".join(rng.choice(list("ACGT"), L))
        for _ in range(100):
            h = list(ref)
            kind, at = int(rng.integers(0, 4)), int(rng.integers(1, L - 1))
            if kind == 0:
                cases.append(from_rows(ref, "".join(h[:at] + ["ACGT"[("ACGT".index(h[at]) + 1) % 4]] + h[at + 1:])))
            elif kind == 1:
                cases.append(from_rows(ref, ref[:at] + "-" + ref[at + 1:]))
            elif kind == 2:
                cases.append(from_rows(ref[:at] + "-" + ref[at:], ref[:at] + "ACGT"[int(rng.integers(0, 4))] + ref[at:]))
            else:
                cases.append(from_rows(ref, ref))
    assert len(cases) == 20000 > 2048 * 4
    got = run_device(cases, 2)
    compare(cases, got, 2)
    assert hapalign.variants_last_launch()["max_draws"] >= 2


def test_a_stream_of_its_own_and_a_second_launch_into_the_same_tensors():
    import torch
    cases = hv.hand_cases() + shape_cases()[:20]
    st = torch.cuda.Stream()
    got = run_device(cases, hv.CAP, stream=st, relaunch=True)
    compare(cases, got, hv.CAP)


def test_the_host_pointer_entry_without_the_slice():
    """dd_align_haplotypes_variants with ref_pos == NULL on the SeqAn fixtures (the device's alignment is the library's, row for row):
    the records of the fixtures' rows; and with the slice, the same records and the slice"""
    cases = hv.fixture_cases()
    refs, haps = [c[0] for c in cases], [c[1] for c in cases]
    want_s, want_v = twin(cases, 8)
    for with_slice in (False, True):
        got = hapalign.align_variants(refs, haps, list(range(len(cases))), cap=8, with_ref_pos=with_slice)
        check_guards()
        assert np.all(got["status"] == 0) and ("ref_pos" in got) == with_slice
        assert np.array_equal(got["summary"], want_s)
        for i in range(len(cases)):
            kept = min(int(want_s[i][0]), 8)
            assert got["variants"][i, :kept].tolist() == want_v[i, :kept].tolist() and not got["variants"][i, kept:].any(), i
        if with_slice:
            assert got["ref_pos"].tolist() == [v for c in cases for v in c[2]]
