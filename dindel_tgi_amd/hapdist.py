"""The block table of a window's empirical haplotype distribution on the device (dd_hap_blocks_compute / dd_hap_blocks_device).

The arithmetic is the library's HIP kernel (csrc/hapdist_kernel.hip); there is no Python implementation behind this module.
`block_table` is the host-pointer entry, `DeviceBlocks` keeps the batch in torch tensors and launches on a given stream, `decode`
turns one window of the flat tables into plain Python structures.

A window is (rs, ref): the 0-based position of its first reference base and the reference bytes; its reads are
[(pos, flag, [(op, len), ...], letters)] in the order the read selection returned them.
"""
import ctypes as C

import numpy as np

from . import capi

WINDOW_FIELDS, OFFSET_FIELDS, TABLE_FIELDS = capi.HAP_BLOCKS_WINDOW_FIELDS, capi.HAP_BLOCKS_OFFSET_FIELDS, capi.HAP_BLOCKS_TABLE_FIELDS
BATCH_FIELDS = ("win_rs", "win_ref_off", "ref_seq", "win_read_off", "read_pos", "read_flag", "read_op_off", "ops", "read_base_off", "bases")


def _csr(lengths):
    return np.concatenate([[0], np.cumsum(lengths, dtype=np.int64)]).astype(np.int32)


def pack(windows, reads):
    """numpy arrays of a dd_hap_batch.  windows: [(rs, ref)], reads: one list of reads per window."""
    if len(reads) != len(windows):
        raise ValueError("one list of reads per window")
    flat = [rd for rs in reads for rd in rs]
    ops = [(ln << 4) | op for rd in flat for op, ln in rd[2]]
    return {"win_rs": np.array([w[0] for w in windows], np.int32), "win_ref_off": _csr([len(w[1]) for w in windows]),
            "ref_seq": np.frombuffer(b"".join(bytes(w[1]) for w in windows), np.uint8).copy(),
            "win_read_off": _csr([len(rs) for rs in reads]),
            "read_pos": np.array([rd[0] for rd in flat], np.int32), "read_flag": np.array([rd[1] for rd in flat], np.int32),
            "read_op_off": _csr([len(rd[2]) for rd in flat]), "ops": np.array(ops, np.uint32),
            "read_base_off": _csr([len(rd[3]) for rd in flat]),
            "bases": np.frombuffer(b"".join(bytes(rd[3]) for rd in flat), np.uint8).copy()}


def _pad(arr):
    """The array itself, or one element of its type: the library wants an address for every array."""
    return arr if arr.size else np.zeros(1, arr.dtype)


def host_batch(a):
    """dd_hap_batch over the numpy arrays of pack() (kept alive in the returned struct's `_keep`)."""
    b = capi.dd_hap_batch()
    b.n_windows, b.n_reads = len(a["win_rs"]), len(a["read_pos"])
    b._keep = {k: _pad(a[k]) for k in BATCH_FIELDS}
    for k in BATCH_FIELDS:
        setattr(b, k, b._keep[k].ctypes.data)
    return b


def offsets(a):
    """The capacities dd_hap_blocks_offsets gives a batch: dict(blk_off, ent_off, ins_off), int32 [n_windows + 1] each."""
    n = len(a["win_rs"])
    o = {k: np.zeros(n + 1, np.int32) for k in OFFSET_FIELDS}
    b = host_batch(a)
    rc = capi.load().dd_hap_blocks_offsets(C.byref(b), *[o[k].ctypes.data for k in OFFSET_FIELDS])
    if rc != 0:
        raise RuntimeError("dd_hap_blocks_offsets: %d %s" % (rc, capi.last_error()))
    return o


def alloc_tables(n_windows, off, fill=0, slack=0):
    """numpy arrays of a dd_hap_blocks for the capacities `off`, every word preset to `fill`; `slack` extra records behind each table."""
    t = {k: np.full(max(n_windows, 1), fill, np.int32) for k in WINDOW_FIELDS}
    t.update({k: np.ascontiguousarray(off[k], np.int32) for k in OFFSET_FIELDS})
    fill_u = np.uint32(fill & 0xffffffff)
    t["blocks"] = np.full(max(int(off["blk_off"][-1]) + slack, 1), fill_u, np.uint32)
    t["entries"] = np.full(2 * max(int(off["ent_off"][-1]) + slack, 1), fill_u, np.uint32)
    t["ins_ops"] = np.full(2 * max(int(off["ins_off"][-1]) + slack, 1), fill_u, np.uint32)
    t["ins_pos"] = np.full(2 * max(int(off["ins_off"][-1]) + slack, 1), fill_u, np.uint32)
    return t


def host_tables(t):
    """dd_hap_blocks over the numpy arrays of alloc_tables() (which must stay alive)."""
    s = capi.dd_hap_blocks()
    for k in WINDOW_FIELDS + OFFSET_FIELDS + TABLE_FIELDS:
        setattr(s, k, t[k].ctypes.data)
    return s


def decode(a, t, w):
    """Window w of the tables as plain structures: dict(status) alone when it is not DD_HAPDIST_OK, else dict(status, blocks, ins, left)
    with blocks = [(start - rs, length, [(bytes, count, is_ref), ...])] in position order and ins = the same (length 0) for the insertion
    positions, sorted by position, the empty reference string first and the inserted strings in byte order."""
    st = int(t["status"][w])
    if st != capi.DD_HAPDIST_OK:
        return {"status": st}
    blocks = []
    e = 2 * int(t["ent_off"][w])
    for k in range(int(t["n_blocks"][w])):
        word = int(t["blocks"][int(t["blk_off"][w]) + k])
        bs, n, cnt, ref_idx = word & 0xffff, (word >> 16) & 15, (word >> 20) & 63, word >> 26
        ent = []
        for i in range(cnt):
            key, count = int(t["entries"][e]), int(t["entries"][e + 1])
            ent.append((key.to_bytes(4, "big")[:n], count, i == ref_idx))
            e += 2
        blocks.append((bs, n, ent))
    io, r0 = 2 * int(t["ins_off"][w]), int(a["win_read_off"][w])
    by_pos = {int(t["ins_pos"][io + 2 * i]): [int(t["ins_pos"][io + 2 * i + 1]), {}] for i in range(int(t["n_ins_pos"][w]))}
    for i in range(int(t["n_ins_ops"][w])):
        r, word = r0 + int(t["ins_ops"][io + 2 * i]), int(t["ins_ops"][io + 2 * i + 1])
        k, at = word >> 16, word & 0xffff
        o0, b0 = int(a["read_op_off"][r]), int(a["read_base_off"][r])
        used = sum(int(c) >> 4 for c in a["ops"][o0:o0 + k] if int(c) & 15 in (0, 1, 4))
        s = a["bases"][b0 + used:b0 + used + (int(a["ops"][o0 + k]) >> 4)].tobytes()
        by_pos[at][1][s] = by_pos[at][1].get(s, 0) + 1
    ins = [(p, 0, [(b"", 1 + by_pos[p][0], True)] + [(s, c, False) for s, c in sorted(by_pos[p][1].items())]) for p in sorted(by_pos)]
    return {"status": st, "blocks": blocks, "ins": ins, "left": int(t["left"][w])}


def block_table(windows, reads, device=0, tables=None):
    """The block tables of `windows` (see the module text) computed on the device.  Returns (a, t): the packed batch and the tables as
    numpy arrays (the fields of dd_hap_blocks; decode(a, t, w) reads one window).  tables: arrays of alloc_tables() to compute into."""
    a = pack(windows, reads)
    t = tables if tables is not None else alloc_tables(len(windows), offsets(a))
    b, s = host_batch(a), host_tables(t)
    rc = capi.load().dd_hap_blocks_compute(C.byref(b), C.byref(s), device)
    if rc != 0:
        raise RuntimeError("dd_hap_blocks_compute: %d %s" % (rc, capi.last_error()))
    return a, t


def last_launch():
    """This thread's last block-table launch: dict(grid, windows, max_draws, guard_trips) (dd_hap_blocks_last_launch; after a
    DeviceBlocks launch the object must still be alive; the call synchronises its stream)."""
    return capi.last_launch_of("dd_hap_blocks_last_launch", capi.HAP_BLOCKS_LOG_FIELDS)


class DeviceBlocks:
    """A batch of windows resident in HBM: torch owns the tensors and the stream, dd_hap_blocks_device does the work."""

    def __init__(self, windows, reads, device="cuda:0", fill=0, slack=0, packed=None):
        """fill, slack: as in alloc_tables (the launch is told the tables' capacities without the slack).  packed: the arrays of pack(),
        made some other way, instead of windows / reads."""
        import torch
        lib = capi.load()
        self.a = packed if packed is not None else pack(windows, reads)
        self.n_windows = len(self.a["win_rs"])
        self.device = torch.device(device)
        self.host = alloc_tables(self.n_windows, offsets(self.a), fill, slack)
        self.t_in = {k: torch.from_numpy(_pad(self.a[k]).view(np.uint8)).to(self.device) for k in BATCH_FIELDS}
        self.t_out = {k: torch.from_numpy(self.host[k].view(np.uint8)).to(self.device) for k in WINDOW_FIELDS + OFFSET_FIELDS + TABLE_FIELDS}
        self.ws_bytes = lib.dd_hap_blocks_workspace_bytes()
        self.workspace = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.device)
        self.batch = capi.dd_hap_batch()
        self.batch.n_windows, self.batch.n_reads = self.n_windows, len(self.a["read_pos"])
        for k in BATCH_FIELDS:
            setattr(self.batch, k, self.t_in[k].data_ptr())
        self.tables = capi.dd_hap_blocks()
        for k, v in self.t_out.items():
            setattr(self.tables, k, v.data_ptr())
        self.caps = [int(self.host["blk_off"][-1]), int(self.host["ent_off"][-1]), int(self.host["ins_off"][-1])]

    def launch(self, stream=None):
        """Enqueue the kernel on `stream` (a torch stream; None = the current one).  Asynchronous."""
        st = capi.stream_of(stream, self.device)
        rc = capi.load().dd_hap_blocks_device(C.byref(self.batch), C.byref(self.tables), self.caps[0], self.caps[1], self.caps[2],
                                              self.workspace.data_ptr(), self.ws_bytes, st.cuda_stream)
        if rc != 0:
            raise RuntimeError("dd_hap_blocks_device: %d %s" % (rc, capi.last_error()))

    def results(self):
        """Synchronise and copy back: (a, t) as block_table returns them."""
        import torch
        torch.cuda.synchronize(self.device)
        t = {k: v.cpu().numpy().view(self.host[k].dtype) for k, v in self.t_out.items()}
        return self.a, t
