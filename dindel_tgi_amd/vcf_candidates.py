"""Candidate indels from a VCF of known sites from Python: ctypes access to host/vcf_candidates.cpp (the reference's convertVCFToDindel.py
with its VCFFile.py, Variant.py and Fasta.py in C++).  No Python implementation behind it."""
import ctypes as C
import json

from . import hostlib


def _json_call(fn, *args):
    cap = 1 << 16
    while True:
        buf = C.create_string_buffer(cap)
        n = fn(*args, buf, cap)
        if n >= 0:
            return json.loads(buf.value.decode())
        cap = -n + 1


def variant4(ref, alt):
    """Variant4 of Variant.py for REF and ALT of unequal lengths: (type, offset, string), e.g. ("del", 1, "-CCC") for ("ACCCT", "AT");
    raises ValueError with the script's text where it raises"""
    lib = hostlib.load()
    lib.ddh_variant4_json.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
    got = _json_call(lib.ddh_variant4_json, ref.encode(), alt.encode())
    if "throw" in got:
        raise ValueError(got["throw"])
    return got["type"], got["offset"], got["str"]


def convert_with_notes(vcf_files, ref_fasta, out, min_qual=1.0, tid=None, region=None):
    """convert(), returning dict(lines=number written, stderr=the script's notes, stdout=its one print, throw=the cause if it died)"""
    lib = hostlib.load()
    lib.ddh_vcf_convert_json.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_double, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
    files = vcf_files if isinstance(vcf_files, str) else ",".join(str(f) for f in vcf_files)
    if (tid is None) != (region is None):
        raise ValueError("tid and region go together")
    enc = lambda s: None if s is None else str(s).encode()
    return _json_call(lib.ddh_vcf_convert_json, files.encode(), str(ref_fasta).encode(), str(out).encode(), float(min_qual), enc(tid), enc(region))


def convert(vcf_files, ref_fasta, out, min_qual=1.0, tid=None, region=None):
    """convertVCFToDindel.py: the indels of the VCF files (a list, or one comma-separated string; plain or .gz) with QUAL `.` or
    >= min_qual go to `out` as `tid pos variant` lines (zero-based), the input of dindel_candidates --analysis realignCandidates.
    tid and region ("A-B"): only the lines of that target with A <= position < B.  Returns the number of lines written; raises
    ValueError with the cause where the script dies."""
    got = convert_with_notes(vcf_files, ref_fasta, out, min_qual, tid, region)
    if "throw" in got:
        raise ValueError(got["throw"])
    return got["lines"]
