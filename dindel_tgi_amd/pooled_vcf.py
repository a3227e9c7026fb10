"""The end of the pooled workflow from Python: ctypes access to host/pooled_vcf.cpp (the reference's mergeOutputPooled.py and
makeGenotypeLikelihoodFilePooled.py in C++).  No Python implementation behind it."""
import ctypes as C
import json

from . import hostlib


def _bytes_kept(x):
    """the C side writes every byte outside printable ASCII as \\u00XX: back to the text those bytes spell"""
    if isinstance(x, str):
        return x.encode("latin-1").decode("utf-8", "surrogateescape")
    return {k: _bytes_kept(v) for k, v in x.items()} if isinstance(x, dict) else x


def _json_call(fn, *args):
    """one call of the C entry; a result larger than the buffer is fetched from the library, the work is not done twice"""
    cap = 1 << 16
    buf = C.create_string_buffer(cap)
    n = fn(*args, buf, cap)
    if n < 0:
        last = hostlib.load().ddh_pooled_last_notes
        last.argtypes = [C.c_char_p, C.c_int]
        buf = C.create_string_buffer(-n + 1)
        assert last(buf, -n + 1) >= 0
    return _bytes_kept(json.loads(buf.value.decode()))


def merge_with_notes(glf_list, ref_fasta, out_vcf, num_samples, num_bam_files=1, max_hp_len=10, filter_fr=False, filter_qual=20):
    """merge(), returning dict(stderr=the script's notes, stdout=its progress lines, throw=the cause if it died)"""
    lib = hostlib.load()
    lib.ddh_pooled_vcf_json.argtypes = [C.c_char_p] * 3 + [C.c_int] * 5 + [C.c_char_p, C.c_int]
    return _json_call(lib.ddh_pooled_vcf_json, str(glf_list).encode(), str(ref_fasta).encode(), str(out_vcf).encode(), int(num_samples), int(num_bam_files),
                      int(max_hp_len), 1 if filter_fr else 0, int(filter_qual))


def merge(glf_list, ref_fasta, out_vcf, num_samples, num_bam_files=1, max_hp_len=10, filter_fr=False, filter_qual=20):
    """mergeOutputPooled.py: the `singlevariant` lines of the .glf.txt files named in `glf_list` (plain or .gz; num_bam_files lines per
    variant) become the VCF `out_vcf` with the filters q<filter_qual>, fr0 (filter_fr), ocr, s50, hp<max_hp_len>, mf and tc10.  Raises
    ValueError with the cause where the script dies."""
    got = merge_with_notes(glf_list, ref_fasta, out_vcf, num_samples, num_bam_files, max_hp_len, filter_fr, filter_qual)
    if "throw" in got:
        raise ValueError(got["throw"])


def make_glf_with_notes(glf_list, call_vcf, out, bam_list):
    """make_glf(), returning dict(stderr=..., stdout=..., throw=the cause if it died)"""
    lib = hostlib.load()
    lib.ddh_pooled_glf_json.argtypes = [C.c_char_p] * 4 + [C.c_char_p, C.c_int]
    return _json_call(lib.ddh_pooled_glf_json, str(glf_list).encode(), str(call_vcf).encode(), str(out).encode(), str(bam_list).encode())


def make_glf(glf_list, call_vcf, out, bam_list):
    """makeGenotypeLikelihoodFilePooled.py: for every site of `call_vcf` (PASS, or q20 with QUAL >= 10) one line
    `tid pos variant L00 L01 L11 NAME` per pool, from the .glf.txt files named in `glf_list`; NAME is the pool's line of `bam_list`.
    Raises ValueError with the cause where the script dies."""
    got = make_glf_with_notes(glf_list, call_vcf, out, bam_list)
    if "throw" in got:
        raise ValueError(got["throw"])


def variant4(ref, alt):
    """Variant4 of Variant.py for any REF and ALT: (type, offset, string); equal lengths give ("snp", index, "X=>Y").  Raises ValueError with
    the script's text where it raises."""
    lib = hostlib.load()
    lib.ddh_variant4_any_json.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
    got = _json_call(lib.ddh_variant4_any_json, ref.encode(), alt.encode())
    if "throw" in got:
        raise ValueError(got["throw"])
    return got["type"], got["offset"], got["str"]


def percentiles(hist, pctiles=(1, 99)):
    """getPercentiles of mergeOutputPooled.py: hist maps a depth to its count"""
    lib = hostlib.load()
    n, m = len(hist), len(pctiles)
    keys = sorted(hist)
    lib.ddh_get_percentiles.argtypes = [C.POINTER(C.c_long), C.POINTER(C.c_long), C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_long)]
    lib.ddh_get_percentiles.restype = None
    out = (C.c_long * m)()
    lib.ddh_get_percentiles((C.c_long * n)(*keys), (C.c_long * n)(*[hist[k] for k in keys]), n, (C.c_int * m)(*pctiles), m, out)
    return list(out)
