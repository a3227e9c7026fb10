"""Step 3 of the workflow from Python: ctypes access to host/windows.cpp (the reference's makeWindows.py and selectCandidates.py in
C++).  No Python implementation behind it."""
import ctypes as C
import json

from . import hostlib


def _call(lines, min_dist, num_windows_per_file, filt, min_count, max_count):
    lib = hostlib.load()
    lib.ddh_make_windows_json.argtypes = [C.c_char_p, C.c_long, C.c_long, C.c_int, C.c_long, C.c_long, C.c_char_p, C.c_int]
    text = "".join(l.rstrip("\n") + "\n" for l in lines).encode()
    cap = 4 * len(text) + (1 << 16)
    while True:
        buf = C.create_string_buffer(cap)
        n = lib.ddh_make_windows_json(text, min_dist, num_windows_per_file, 1 if filt else 0, min_count, max_count, buf, cap)
        if n >= 0:
            break
        cap = -n + 1
    got = json.loads(buf.value.decode())
    if "throw" in got:
        raise ValueError(got["throw"])
    return got


def _filter_args(min_count, max_count):
    filt = min_count is not None or max_count is not None
    return filt, 2 if min_count is None else min_count, 10000000 if max_count is None else max_count


def make_window_files(lines, min_dist=20, num_windows_per_file=1000, min_count=None, max_count=None):
    """candidate lines (`tid pos variant ... # count ...`) -> {N: [window lines]} for the files PREFIX.N.txt of makeWindows.py;
    min_count / max_count: selectCandidates first (given one, the other takes the script's default)"""
    got = _call(lines, min_dist, num_windows_per_file, *_filter_args(min_count, max_count))
    return {f["number"]: f["lines"] for f in got["files"]}


def make_windows(lines, min_dist=20, num_windows_per_file=1000, min_count=None, max_count=None):
    """the same as one list: every window line (`tid leftPos rightPos pos,variant ...`) in file order"""
    files = make_window_files(lines, min_dist, num_windows_per_file, min_count, max_count)
    return [l for n in sorted(files) for l in files[n]]


def cluster_keys(positions, min_dist):
    """clusterKeys: the cluster key (first position of its single-linkage run) of every one of the sorted distinct positions"""
    lib = hostlib.load()
    lib.ddh_cluster_keys.argtypes = [C.POINTER(C.c_long), C.c_int, C.c_long, C.POINTER(C.c_long)]
    n = len(positions)
    src, dst = (C.c_long * max(n, 1))(*positions), (C.c_long * max(n, 1))()
    lib.ddh_cluster_keys(src, n, min_dist, dst)
    return list(dst[:n])


def select_candidates(lines, min_count=2, max_count=10000000):
    """selectCandidates.py: `tid pos variant # count` lines of the variants seen min_count ... max_count times"""
    lib = hostlib.load()
    lib.ddh_select_candidates_json.argtypes = [C.c_char_p, C.c_long, C.c_long, C.c_char_p, C.c_int]
    text = "".join(l.rstrip("\n") + "\n" for l in lines).encode()
    cap = 4 * len(text) + (1 << 16)
    buf = C.create_string_buffer(cap)
    assert lib.ddh_select_candidates_json(text, min_count, max_count, buf, cap) >= 0
    got = json.loads(buf.value.decode())
    if "throw" in got:
        raise ValueError(got["throw"])
    return got["selected"]
