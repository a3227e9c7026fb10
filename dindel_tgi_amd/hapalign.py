"""alignHaplotypes on the device: candidate haplotypes against their window's reference sequence (dd_align_haplotypes).

The arithmetic is the library's HIP kernel (csrc/hapalign_kernel.hip); there is no Python or CPU implementation behind this module.
`align_haplotypes` is the host-pointer entry, `align_events` the one that brings back indel events (csrc/align_events_kernel.hip)
instead of the per-base slice, `align_variants` the one that brings back every variant with its flanks (csrc/hap_variants_kernel.hip),
`DeviceAlign` keeps the batch in torch tensors and launches on a given stream, and
`gapped_rows` rebuilds the two gapped rows of an alignment from the per-base reference offsets the kernel returns.
"""
import ctypes as C

import numpy as np

from . import capi

_DNA = np.zeros(256, np.uint8)                    # seqan::Dna of a byte: every other byte is an A
for _c, _v in (("C", 1), ("G", 2), ("T", 3), ("U", 3)):
    _DNA[ord(_c)] = _DNA[ord(_c.lower())] = _v


def dna_text(seq):
    """The sequence as the alignment sees it: ACGT of the bytes' seqan::Dna codes."""
    return np.frombuffer(b"ACGT", np.uint8)[_DNA[np.frombuffer(bytes(seq), np.uint8)]].tobytes().decode()


def pack(refs, haps, pair_ref):
    """numpy arrays of a dd_align_batch: ref_off, ref_seq, pair_ref, hap_off, hap_seq."""
    refs, haps = [bytes(r) for r in refs], [bytes(h) for h in haps]
    if len(pair_ref) != len(haps):
        raise ValueError("one pair_ref entry per haplotype")
    a = {"ref_off": np.concatenate([[0], np.cumsum([len(r) for r in refs], dtype=np.int64)]).astype(np.int32),
         "hap_off": np.concatenate([[0], np.cumsum([len(h) for h in haps], dtype=np.int64)]).astype(np.int32),
         "pair_ref": np.ascontiguousarray(pair_ref, np.int32),
         "ref_seq": np.frombuffer(b"".join(refs), np.uint8).copy(), "hap_seq": np.frombuffer(b"".join(haps), np.uint8).copy()}
    return a


def _struct(a, addr):
    b = capi.dd_align_batch()
    b.n_refs, b.n_pairs = len(a["ref_off"]) - 1, len(a["hap_off"]) - 1
    for k in ("ref_off", "ref_seq", "pair_ref", "hap_off", "hap_seq"):
        setattr(b, k, addr(a[k]))
    return b


def _host_addr(arr):
    return arr.ctypes.data if arr.size else None


def host_batch(a):
    """dd_align_batch over the numpy arrays of pack() (which must stay alive)."""
    return _struct(a, _host_addr)


def _host_call(symbol, refs, haps, pair_ref, device, with_ref_pos, extra=(), cap=None):
    """One host-pointer entry: pack, allocate, call, raise, slice.  extra: (key, dtype, trailing shape) of the arrays the entry takes
    behind the result, in its argument order, followed by `cap`.  ref_pos is part of the result only with_ref_pos."""
    a = pack(refs, haps, pair_ref)
    n, nb = len(haps), int(a["hap_off"][-1])
    out = {"score": np.zeros(max(n, 1), np.int32), "status": np.zeros(max(n, 1), np.int32), "ref_pos": np.zeros(max(nb, 1), np.int16)}
    out.update({k: np.zeros((max(n, 1),) + shape, dt) for k, dt, shape in extra})
    b = host_batch(a)
    r = capi.dd_align_result(out["score"].ctypes.data, out["status"].ctypes.data, out["ref_pos"].ctypes.data if with_ref_pos else None)
    args = [out[k].ctypes.data for k, _, _ in extra] + ([int(cap)] if extra else [])
    rc = getattr(capi.load(), symbol)(C.byref(b), C.byref(r), *args, device)
    if rc != 0:
        raise RuntimeError("%s: %d %s" % (symbol, rc, capi.last_error()))
    res = {k: out[k][:n] for k in ["score", "status"] + [k for k, _, _ in extra]}
    res["hap_off"] = a["hap_off"]
    if with_ref_pos:
        res["ref_pos"] = out["ref_pos"][:nb]
    return res


def align_haplotypes(refs, haps, pair_ref, device=0):
    """Align haps[i] (bytes) globally against refs[pair_ref[i]].  Returns dict(score int32 [n], status int32 [n], ref_pos int16 laid
    out like the concatenated haplotypes, hap_off int32 [n + 1]): ref_pos[hap_off[i] + b] is the 0-based offset of the reference
    base that base b of haplotype i is paired with, or -1 - n when it faces a gap, n = the number of reference bases left of its column."""
    return _host_call("dd_align_haplotypes", refs, haps, pair_ref, device, True)


EVENT_FIELDS = ("kind", "ref", "len", "hap")


def align_events(refs, haps, pair_ref, events_cap=8, device=0, with_ref_pos=False):
    """Align like align_haplotypes and return the indel events of every pair instead of its slice: dict(score, status, n_events int32
    [n], events int16 [n, events_cap, 4] with the fields of EVENT_FIELDS, hap_off).  n_events is the true count; a pair with
    n_events > events_cap holds its first events_cap records.  with_ref_pos=True also copies the slice back (ref_pos)."""
    extra = (("n_events", np.int32, ()), ("events", np.int16, (max(int(events_cap), 1), 4)))
    return _host_call("dd_align_haplotypes_events", refs, haps, pair_ref, device, with_ref_pos, extra, events_cap)


def events_last_launch():
    """This thread's last event launch: dict(grid, pairs, max_draws, guard_trips) (dd_align_events_last_launch)."""
    return capi.last_launch_of("dd_align_events_last_launch", capi.ALIGN_EVENTS_LOG_FIELDS)


VARIANT_FIELDS = ("kind", "key", "len", "start_read", "left_flank_hap", "right_flank_hap", "left_flank_read", "right_flank_read")
SUMMARY_FIELDS = ("n_variants", "first_base", "last_base", "flags")


def align_variants(refs, haps, pair_ref, cap=16, device=0, with_ref_pos=False):
    """Align like align_haplotypes and return every pair's variants instead of its slice: dict(score, status, summary int32 [n, 4] with
    the fields of SUMMARY_FIELDS, variants int16 [n, cap, 8] with the fields of VARIANT_FIELDS, hap_off).  n_variants is the true count;
    a pair with more than `cap` holds its first `cap` records.  with_ref_pos=True also copies the slice back (ref_pos)."""
    extra = (("summary", np.int32, (4,)), ("variants", np.int16, (max(int(cap), 1), 8)))
    return _host_call("dd_align_haplotypes_variants", refs, haps, pair_ref, device, with_ref_pos, extra, cap)


def variants_last_launch():
    """This thread's last variants launch: dict(grid, pairs, max_draws, guard_trips) (dd_hap_variants_last_launch)."""
    return capi.last_launch_of("dd_hap_variants_last_launch", capi.ALIGN_EVENTS_LOG_FIELDS)


def gapped_rows(ref, hap, ref_pos):
    """The two gapped rows (reference, haplotype) of one alignment, as SeqAn prints them: ACGT of the converted bases, '-' for a gap.
    ref_pos: the pair's slice of the result.  A base that faces a gap carries -1 - n, n = the reference bases left of its column
    (DD_ALIGN_GAP_REFS), which is what orders it against deleted reference bases next to it."""
    r, h = dna_text(ref), dna_text(hap)
    row0, row1, nxt = [], [], 0
    for b, p in enumerate(np.asarray(ref_pos).tolist()):
        upto = p if p >= 0 else -1 - p                   # reference bases in front of this column: deleted ones first
        if not nxt <= upto <= len(r) - (p >= 0):
            raise ValueError("ref_pos does not describe an alignment")
        row0.append(r[nxt:upto]); row1.append("-" * (upto - nxt))
        nxt = upto
        if p < 0:
            row0.append("-"); row1.append(h[b])
        else:
            row0.append(r[p]); row1.append(h[b])
            nxt = p + 1
    row0.append(r[nxt:]); row1.append("-" * (len(r) - nxt))
    return "".join(row0), "".join(row1)


def last_launch():
    """This thread's last alignment launch: dict(grid, waves, tile_bytes, lds_block, pairs, ws_bytes, max_draws, guard_trips); the last
    two come from the workspace header (after a DeviceAlign launch the object must still be alive; the call synchronises its stream)."""
    return capi.last_launch_of("dd_align_last_launch", capi.ALIGN_LOG_FIELDS)


class DeviceAlign:
    """An alignment batch resident in HBM: torch owns the tensors and the stream, dd_align_haplotypes_device does the work."""

    def __init__(self, refs, haps, pair_ref, device="cuda:0", max_workgroups=None):
        """max_workgroups: give the launch a workspace for no more than that many workgroups (the grid follows the workspace); None = the
        full grid of dd_align_workspace_bytes."""
        import torch
        from .device import _to_dev
        lib = capi.load()
        self.a = pack(refs, haps, pair_ref)
        self.n_pairs = len(haps)
        self.hap_bytes = int(self.a["hap_off"][-1])
        self.device = torch.device(device)
        hb = host_batch(self.a)
        self.ws_bytes = lib.dd_align_workspace_bytes(C.byref(hb))
        if self.ws_bytes == 0:
            raise ValueError("dd_align_workspace_bytes: " + capi.last_error())
        lim = capi.DD_LONG_MAX_HAP_LEN
        rl, hl = np.diff(self.a["ref_off"]), np.diff(self.a["hap_off"])
        self.max_ref_len = max(int(rl[rl <= lim].max(initial=1)), 1)
        self.max_hap_len = max(int(hl[hl <= lim].max(initial=1)), 1)
        if max_workgroups is not None:
            tile = ((self.max_ref_len + 64) * self.max_hap_len + 255) // 256 * 256
            self.ws_bytes = min(self.ws_bytes, 256 + 4 * tile * max(int(max_workgroups), 1))
        self.t = {k: _to_dev(v, self.device) for k, v in self.a.items()}
        self.score = torch.zeros(max(self.n_pairs, 1), dtype=torch.int32, device=self.device)
        self.status = torch.zeros(max(self.n_pairs, 1), dtype=torch.int32, device=self.device)
        self.ref_pos = torch.zeros(max(self.hap_bytes, 1), dtype=torch.int16, device=self.device)
        self.workspace = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.device)
        self.batch = _struct(self.t, lambda t: t.data_ptr())
        self.result = capi.dd_align_result(self.score.data_ptr(), self.status.data_ptr(), self.ref_pos.data_ptr())

    def launch(self, stream=None):
        """Enqueue the alignment on `stream` (a torch stream; None = the current one).  Asynchronous."""
        st = capi.stream_of(stream, self.device)
        rc = capi.load().dd_align_haplotypes_device(C.byref(self.batch), C.byref(self.result), self.max_ref_len, self.max_hap_len,
                                                    self.workspace.data_ptr(), self.ws_bytes, st.cuda_stream)
        if rc != 0:
            raise RuntimeError("dd_align_haplotypes_device: %d %s" % (rc, capi.last_error()))

    def results(self):
        """Synchronise and copy back: the dict align_haplotypes returns."""
        import torch
        torch.cuda.synchronize(self.device)
        return {"score": self.score.cpu().numpy()[:self.n_pairs], "status": self.status.cpu().numpy()[:self.n_pairs],
                "ref_pos": self.ref_pos.cpu().numpy()[:self.hap_bytes], "hap_off": self.a["hap_off"]}

    def _launch_behind(self, symbol, counts, records, width, cap, stream, fill):
        """Enqueue `symbol` (the event or the variants extraction) behind launch() on the same stream.  counts, records: the attributes
        of its two tensors, int32 [n_pairs] + counts' shape and int16 [n_pairs, cap, width]; made on first use or when cap changes,
        and preset (counts to 0, records to `fill`) unless fill is None."""
        import torch
        st = capi.stream_of(stream, self.device)
        c, n = max(int(cap), 1), max(self.n_pairs, 1)
        with torch.cuda.stream(st):
            if getattr(self, records, None) is None or getattr(self, records).shape[1] != c:
                setattr(self, counts[0], torch.zeros((n,) + counts[1], dtype=torch.int32, device=self.device))
                setattr(self, records, torch.zeros((n, c, width), dtype=torch.int16, device=self.device))
            if fill is not None:
                getattr(self, counts[0]).zero_()
                getattr(self, records).fill_(fill)
        rc = getattr(capi.load(), symbol)(C.byref(self.batch), C.byref(self.result), getattr(self, counts[0]).data_ptr(),
                                          getattr(self, records).data_ptr(), int(cap), st.cuda_stream)
        if rc != 0:
            raise RuntimeError("%s: %d %s" % (symbol, rc, capi.last_error()))

    def launch_events(self, events_cap=8, stream=None, fill=0):
        """Enqueue the event extraction behind launch() on the same stream: fills self.n_events (int32 [n_pairs]) and self.events
        (int16 [n_pairs, events_cap, 4]).  The kernel writes only the records it counts; the rest of self.events is preset to `fill`
        (None: left as it is, the tensors of the previous call are reused).  Asynchronous."""
        self._launch_behind("dd_align_events_device", ("n_events", ()), "events", 4, events_cap, stream, fill)

    def event_results(self):
        """Synchronise and copy back n_events and events of the last launch_events()."""
        import torch
        torch.cuda.synchronize(self.device)
        return {"n_events": self.n_events.cpu().numpy()[:self.n_pairs], "events": self.events.cpu().numpy()[:self.n_pairs]}

    def launch_variants(self, cap=16, stream=None, fill=0):
        """Enqueue the variant extraction behind launch() on the same stream: fills self.summary (int32 [n_pairs, 4]) and self.variants
        (int16 [n_pairs, cap, 8]).  The kernel writes only the records it counts; the rest of self.variants is preset to `fill`
        (None: left as it is, the tensors of the previous call are reused).  Asynchronous."""
        self._launch_behind("dd_hap_variants_device", ("summary", (4,)), "variants", 8, cap, stream, fill)

    def variant_results(self):
        """Synchronise and copy back summary and variants of the last launch_variants()."""
        import torch
        torch.cuda.synchronize(self.device)
        return {"summary": self.summary.cpu().numpy()[:self.n_pairs], "variants": self.variants.cpu().numpy()[:self.n_pairs]}
