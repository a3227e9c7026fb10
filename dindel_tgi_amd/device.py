"""Device-resident batches: torch owns HBM and the stream, the C ABI (dd_launch_device) does the work.

PyTorch is plumbing here (allocation, streams, torch.distributed); no torch op touches the data path.
"""
import ctypes as C

import numpy as np
import torch

from . import capi
from .batch import PackedBatch, RESULT_DTYPES, result_lengths

_TORCH_DT = {np.dtype(np.float64): torch.float64, np.dtype(np.uint8): torch.uint8, np.dtype(np.int16): torch.int16,
             np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64}


def _to_dev(arr, device):
    a = np.ascontiguousarray(arr)
    if a.dtype == np.uint32:                      # torch has no uint32 arithmetic; ship the bits as int32
        a = a.view(np.int32)
    if a.size == 0:
        a = np.zeros(1, a.dtype)
    if not a.flags.writeable:
        a = a.copy()
    return torch.from_numpy(a).to(device, non_blocking=False)


class DeviceBatch:
    """A PackedBatch resident in HBM + the dd_device_batch that points at it."""

    def __init__(self, pb: PackedBatch, params: capi.dd_params, device="cuda:0", long_windows=False, long_windows_faster=False,
                 cigars=False, ops_cap=capi.DD_CIGAR_DEFAULT_OPS_CAP, hap_ref_pos=None, hap_aligned=None, realign=False, hap_n_indels=None,
                 diploid_prior=None, indel_keys=False, audit=0, audit_seed=0, audit_max_records=256, audit_faster=0,
                 wide_deletions=False, wide_deletions_faster=False):
        """long_windows: windows beyond the main kernels' limits (haplotypes up to 4,094 bp, reads up to 4,096 bp, and with maxLengthDel
        12..31 haplotypes over 574 bp) are computed by the long-window kernel after the main launch (dd_launch_device_long) instead of
        being marked DD_PAIR_UNSUPPORTED.  Off by default.
        long_windows_faster: the same for the --faster model: the batch is screened for that model (haplotypes over 766 bp or reads over
        1,024 bp, within the same long limits), and launch_faster() follows its main launch with dd_launch_device_faster_long.  A resident
        batch is screened once, for one model: both flags together raise ValueError, and launch() on such a batch raises.
        cigars: launch_cigars() turns the pairs' hpos into CIGARs on the device (dd_cigars_device) and results() also returns cigar_n_ops,
        cigar_ops [n_pairs, ops_cap], cigar_ref_off and cigar_status.  hap_ref_pos: Haplotype::refHpos, one int32 per haplotype base
        (laid out like hap_seq); hap_aligned: one byte per haplotype, 0 = not aligned (None = all aligned).  Off by default.
        realign: launch_realign() chooses the haplotype each read is realigned to and computes that pair's CIGAR alone (dd_realign_device);
        results() also returns realign_hap, realign_status, realign_n_ops, realign_ops [n_reads, ops_cap] and realign_ref_off.  Needs
        hap_ref_pos like cigars; hap_n_indels (Haplotype::countIndels per haplotype) is needed by the DD_REALIGN_PAIR rule only.
        diploid_prior: getHaplotypePrior per haplotype pair, H * H doubles per window (dd_pair_sum_offsets' layout): launch_diploid_pairs()
        picks and certifies every window's MAP haplotype pair on the device (dd_diploid_pairs_device); its `pair` tensor can be handed to
        launch_realign(DD_REALIGN_PAIR, ...) as it is, and diploid_pair_results() copies the per-window outputs back.
        indel_keys: launch_indel_keys() counts the distinct indel-map keys of every pair of the --faster model on the device
        (dd_indel_keys_device) from the hpos of the last launch_faster(), and results() also returns indel_keys (int16 [n_pairs]: the
        count, DD_INDEL_KEYS_OVERFLOW or DD_INDEL_KEYS_NOT_COMPUTED).  Off by default.
        audit: that many of the batch's ordinary windows (chosen once, with audit_seed: dd_audit_select) are recomputed by the long-window
        kernel into shadow tensors as large as the sample and compared bit for bit on the device with what launch() left in HBM:
        launch_audit() behind launch(), audit_results() for the counts, the first audit_max_records differences and the shadow.  Main
        model only (ValueError with long_windows_faster).  0 = off.
        audit_faster: the same for the --faster model: that many of the windows launch_faster() computes (the long ones too with
        long_windows_faster; dd_audit_select_faster, audit_seed) are recomputed by the independent shadow kernel
        (dd_audit_device_faster) and compared with what launch_faster() left in HBM: launch_audit_faster() behind launch_faster(),
        audit_faster_results() in audit_results()' dict shape.  ValueError with long_windows (the batch is then screened for the main
        model).  0 = off.
        wide_deletions: params.maxLengthDel above 31 is accepted (DD_OPT_WIDE_DELETIONS): launch() then sends every window through the
        long-window kernel's wide build (dd_launch_device_wide, no main launch; windows beyond the long limits get their placeholders from
        it).  Needs long_windows (ValueError without); with maxLengthDel <= 31 it changes nothing.  No audit with maxLengthDel above 31.
        wide_deletions_faster: the same value lifted for launch_faster() (dd_launch_device_faster_ex; the --faster model only compares it
        with the haplotype length).  Not with long_windows; the long windows of the --faster model take such a value through the
        host-pointer entries only (dd_compute_likelihoods_faster_ex)."""
        if wide_deletions and not long_windows:
            raise ValueError("wide_deletions needs long_windows=True: the wide build is the long-window kernel's")
        if wide_deletions_faster and (long_windows or long_windows_faster):
            raise ValueError("wide_deletions_faster lifts the check for launch_faster()'s main launch: not with long_windows / long_windows_faster")
        self.opt_wide = capi.DD_OPT_WIDE_DELETIONS if (wide_deletions or wide_deletions_faster) else 0
        self.wide = bool(wide_deletions) and params.maxLengthDel > capi.DD_MAX_LENGTH_DEL
        if long_windows and long_windows_faster:
            raise ValueError("long_windows and long_windows_faster screen the batch for different models: one resident batch, one screening")
        lib = capi.load()
        self.pb, self.params, self.device = pb, params, torch.device(device)
        self.long_windows = bool(long_windows)
        self.long_windows_faster = bool(long_windows_faster)
        a = pb.a
        t = {}
        for k in ["win_hap_off", "win_read_off", "win_hap_start", "hap_seq_off", "hap_seq", "hap_var_off", "hap_var",
                  "read_seq_off", "read_seq", "read_qidx", "read_mqidx", "read_start", "read_flags"]:
            t[k] = _to_dev(a[k], self.device)
        hb = pb.ctypes_batch()
        hap_window = np.zeros(max(pb.n_haps, 1), np.int32)
        po = np.zeros(pb.n_windows + 1, np.int64); ho = np.zeros_like(po); vo = np.zeros_like(po)
        rc = lib.dd_build_index(C.byref(hb), hap_window.ctypes.data_as(capi.c_i32p), po.ctypes.data_as(capi.c_i64p),
                                ho.ctypes.data_as(capi.c_i64p), vo.ctypes.data_as(capi.c_i64p))
        if rc != 0:
            raise RuntimeError("dd_build_index: " + capi.last_error())
        tables = np.zeros(capi.DD_TABLE_DOUBLES, np.float64)
        rc = lib.dd_build_tables_ex(C.byref(params), hb.qual_table, hb.n_qual, hb.mapq_table, hb.n_mapq,
                                    tables.ctypes.data_as(capi.c_f64p), self.opt_wide)
        if rc < 0:
            raise RuntimeError("dd_build_tables_ex: " + capi.last_error())
        t["hap_window"] = _to_dev(hap_window, self.device)
        t["win_pair_off"] = _to_dev(po, self.device)
        t["win_hpos_off"] = _to_dev(ho, self.device)
        t["win_varcov_off"] = _to_dev(vo, self.device)
        t["tables"] = _to_dev(tables, self.device)
        lut = np.zeros(256, np.uint8)
        if lib.dd_build_symbol_lut(C.byref(hb), lut.ctypes.data_as(C.POINTER(C.c_uint8))) != 0:
            raise RuntimeError("dd_build_symbol_lut: " + capi.last_error())
        t["sym_lut"] = _to_dev(lut, self.device)
        if pb.mate is not None and params.mapUnmappedReads:
            lp = np.zeros(max(len(pb.mate["lib_prob"]), 1)); l95 = np.zeros(len(pb.mate["lib_p95"]))
            if lib.dd_build_library_tables(C.byref(hb), lp.ctypes.data_as(capi.c_f64p), l95.ctypes.data_as(capi.c_f64p)) != 0:
                raise RuntimeError("dd_build_library_tables: " + capi.last_error())
            for k in ("read_mate_pos", "read_mate_len", "read_lib", "lib_off"):
                t[k] = _to_dev(pb.mate[k], self.device)
            t["lib_logprob"] = _to_dev(lp, self.device)
            t["lib_log95"] = _to_dev(l95, self.device)
        if pb.hap_var_flank is not None and len(pb.hap_var_flank):
            t["hap_var_flank"] = _to_dev(pb.hap_var_flank, self.device)
        # ragged batches: per-class launch plans (haplotype length x read length), as the host-pointer path does by itself
        # windows outside the kernel limits are marked (DD_PAIR_UNSUPPORTED), not computed: flags + the maxima of the rest
        skip = np.zeros(max(pb.n_windows, 1), np.uint8)
        self.n_long = 0
        if self.long_windows or self.long_windows_faster:   # classes: 0 main kernels, 1 unsupported, 2 long path (the main kernels skip every non-zero value)
            ok_max = (C.c_int32 * 4)()
            opt = (capi.DD_OPT_LONG_WINDOWS_FASTER if self.long_windows_faster else capi.DD_OPT_LONG_WINDOWS) | self.opt_wide
            n_bad = lib.dd_screen_windows_ex(C.byref(params), C.byref(hb), opt, skip.ctypes.data_as(capi.c_u8p),
                                             C.byref(ok_max))
            if n_bad < 0:
                raise RuntimeError("dd_screen_windows_ex: " + capi.last_error())
            self.n_long = int((skip[:pb.n_windows] == capi.DD_WIN_LONG).sum())
            self.n_skipped = n_bad + self.n_long
        else:
            ok_max = (C.c_int32 * 2)()
            self.n_skipped = lib.dd_screen_windows(C.byref(hb), skip.ctypes.data_as(capi.c_u8p), C.byref(ok_max))
            if self.n_skipped < 0:
                raise RuntimeError("dd_screen_windows: " + capi.last_error())
        if self.n_skipped:
            t["win_skip"] = _to_dev(skip, self.device)
        self.classes = capi.dd_length_classes()
        hcl = np.zeros(max(pb.n_haps, 1) * capi.N_READ_CLASSES, np.int32)
        # (launch classes are the main kernels': none where maxLengthDel is beyond every main build)
        if params.maxLengthDel <= capi.DD_MAX_LENGTH_DEL and \
           lib.dd_build_length_classes(C.byref(hb), skip.ctypes.data_as(capi.c_u8p) if self.n_skipped else None, C.byref(params),
                                       hcl.ctypes.data_as(capi.c_i32p), C.byref(self.classes)) != 0:
            raise RuntimeError("dd_build_length_classes: " + capi.last_error())
        t["hap_class_list"] = _to_dev(hcl[:max(self.classes.list_len, 1)], self.device)
        self.t = t
        db = capi.dd_device_batch()
        db.n_windows, db.n_haps, db.n_reads = pb.n_windows, pb.n_haps, pb.n_reads
        db.max_hap_len, db.max_read_len = max(int(ok_max[0]), 1), max(int(ok_max[1]), 1)
        nr = np.diff(a["win_read_off"])
        db.max_window_reads = int(nr[skip[:pb.n_windows] == 0].max()) if pb.n_windows and (skip[:pb.n_windows] == 0).any() else 0
        for k, v in t.items():
            setattr(db, k, v.data_ptr())
        db.n_qual, db.n_mapq = hb.n_qual, hb.n_mapq
        db.classes = C.addressof(self.classes)
        if self.n_long:
            db.long_max_hap_len, db.long_max_read_len = int(ok_max[2]), int(ok_max[3])
        self.db = db
        # results
        n = result_lengths(pb)
        self.out = {k: torch.zeros(max(n[k], 1), dtype=_TORCH_DT[np.dtype(RESULT_DTYPES[k])], device=self.device)
                    for k, _ in capi.RESULT_FIELDS}
        dr = capi.dd_device_result()
        for k, _ in capi.RESULT_FIELDS:
            setattr(dr, k, self.out[k].data_ptr())
        self.dr = dr
        self._n = n
        # device scratch the launch needs for this shape (back-pointer tiles in HBM for long reads); 0 if none
        self.ws_bytes = int(lib.dd_workspace_bytes(C.byref(params), C.byref(db)))
        self.ws = torch.empty(max(self.ws_bytes, 8), dtype=torch.uint8, device=self.device)
        ws_long = lib.dd_workspace_bytes_faster_long if self.long_windows_faster else lib.dd_workspace_bytes_wide if self.wide else lib.dd_workspace_bytes_long
        self.long_ws_bytes = int(ws_long(C.byref(params), C.byref(db))) if self.n_long else 0
        self.long_ws = torch.empty(max(self.long_ws_bytes, 8), dtype=torch.uint8, device=self.device) if (self.n_long or self.wide) else None
        self.cigars = bool(cigars)
        self.realign = bool(realign)
        if self.cigars or self.realign:
            if hap_ref_pos is None:
                raise ValueError("cigars=True and realign=True need hap_ref_pos (Haplotype::refHpos per haplotype base)")
            hrp = np.ascontiguousarray(hap_ref_pos, np.int32)
            if hrp.shape != (int(a["hap_seq_off"][pb.n_haps]),):
                raise ValueError("hap_ref_pos must hold one entry per haplotype base")
            if ops_cap < 1:
                raise ValueError("ops_cap must be at least 1")
            self.ops_cap = int(ops_cap)
            t["hap_ref_pos"] = _to_dev(hrp, self.device)
            if hap_aligned is not None:
                hal = np.ascontiguousarray(hap_aligned, np.uint8)
                if hal.shape != (pb.n_haps,):
                    raise ValueError("hap_aligned must hold one byte per haplotype")
                t["hap_aligned"] = _to_dev(hal, self.device)
        if self.realign:
            if hap_n_indels is not None:
                hni = np.ascontiguousarray(hap_n_indels, np.int32)
                if hni.shape != (pb.n_haps,):
                    raise ValueError("hap_n_indels must hold one entry per haplotype")
                t["hap_n_indels"] = _to_dev(hni, self.device)
            nread = max(pb.n_reads, 1)
            self.rl = {k: torch.zeros(nread * (self.ops_cap if k == "ops" else 1), dtype=torch.int32, device=self.device)
                       for k in capi.REALIGN_RESULT_FIELDS}                                                 # ops: uint32 bits
            self.drl = capi.dd_realign_result(*[self.rl[k].data_ptr() for k in capi.REALIGN_RESULT_FIELDS])
        self.dip = None
        if diploid_prior is not None:
            hh = np.zeros(pb.n_windows + 1, np.int64)
            hh[1:] = np.cumsum(np.diff(a["win_hap_off"]).astype(np.int64) ** 2)
            pr = np.ascontiguousarray(diploid_prior, np.float64).reshape(-1)
            if pr.shape != (int(hh[-1]),):
                raise ValueError("diploid_prior must hold H * H entries per window")
            t["win_hh_off"] = _to_dev(hh, self.device)
            t["diploid_prior"] = _to_dev(pr, self.device)
            nwin = max(pb.n_windows, 1)
            self.dip = {k: torch.zeros(nwin * (2 if k == "pair" else 1), dtype=_TORCH_DT[np.dtype(capi.DIPLOID_PAIR_DTYPES[k])], device=self.device)
                        for k in capi.DIPLOID_PAIR_FIELDS}
            self.ddip = capi.dd_diploid_pair_result(*[self.dip[k].data_ptr() for k in capi.DIPLOID_PAIR_FIELDS])
        self.indel_keys = bool(indel_keys)
        if self.indel_keys:
            self.keys = torch.zeros(max(pb.n_pairs, 1), dtype=torch.int16, device=self.device)
        self.audit = None
        if audit and int(audit) > 0:
            if self.wide:
                raise ValueError("no audit with maxLengthDel above 31: the shadow would be the same kernel")
            if self.long_windows_faster:
                raise ValueError("audit checks the main model against its long-window kernel: not with long_windows_faster")
            smp = capi.AuditSample(params, pb, int(audit), audit_seed, skip[:pb.n_windows] if self.n_skipped else None)
            self.audit = smp
            self.audit_max_records = int(audit_max_records)
            at = [_to_dev(a, self.device) for a in (smp.audit_class, smp.pair_off, smp.hpos_off, smp.varcov_off)]
            self._audit_t = at
            self.audit_view = smp.view([x.data_ptr() for x in at])
            sn = {"hpos": smp.sizes.hpos_len, "var_covered": smp.sizes.var_cov_len, "var_fcov": smp.sizes.var_cov_len, "onHap": 0}
            self._shadow_n = {k: int(sn.get(k, smp.sizes.n_pairs)) for k, _ in capi.RESULT_FIELDS}
            self.shadow = {k: torch.zeros(max(self._shadow_n[k], 1), dtype=_TORCH_DT[np.dtype(RESULT_DTYPES[k])], device=self.device)
                           for k, _ in capi.RESULT_FIELDS if k != "onHap"}
            self.dshadow = capi.dd_device_result()
            for k, v in self.shadow.items():
                setattr(self.dshadow, k, v.data_ptr())
            self.audit_report_t = torch.zeros(len(capi.audit_report_buffer(self.audit_max_records)) // 8, dtype=torch.int64, device=self.device)
            self.audit_ws_bytes = int(lib.dd_audit_workspace_bytes(C.byref(params), C.byref(self.audit_view)))
            self.audit_ws = torch.empty(max(self.audit_ws_bytes, 8), dtype=torch.uint8, device=self.device)
        self.audit_faster = None
        if audit_faster and int(audit_faster) > 0:
            if self.long_windows:
                raise ValueError("audit_faster checks what launch_faster() computes: not with long_windows (the main model's screen)")
            smp = capi.AuditSample(params, pb, int(audit_faster), audit_seed, skip[:pb.n_windows] if self.n_skipped else None, faster=True,
                                   options=capi.DD_OPT_LONG_WINDOWS_FASTER if self.long_windows_faster else 0)
            self.audit_faster = smp
            self.audit_max_records = int(audit_max_records)
            self._audit_faster_t = [_to_dev(x, self.device) for x in (smp.audit_class, smp.pair_off, smp.hpos_off, smp.varcov_off)]
            self.audit_faster_view = smp.view([x.data_ptr() for x in self._audit_faster_t])
            sn = {"hpos": smp.sizes.hpos_len, "var_covered": smp.sizes.var_cov_len, "var_fcov": smp.sizes.var_cov_len, "onHap": 0}
            self._shadow_faster_n = {k: int(sn.get(k, smp.sizes.n_pairs)) for k, _ in capi.RESULT_FIELDS}
            self.shadow_faster = {k: torch.zeros(max(self._shadow_faster_n[k], 1), dtype=_TORCH_DT[np.dtype(RESULT_DTYPES[k])], device=self.device)
                                  for k, _ in capi.RESULT_FIELDS if k != "onHap"}
            self.dshadow_faster = capi.dd_device_result()
            for k, v in self.shadow_faster.items():
                setattr(self.dshadow_faster, k, v.data_ptr())
            self.audit_faster_report_t = torch.zeros(len(capi.audit_report_buffer(self.audit_max_records)) // 8, dtype=torch.int64,
                                                     device=self.device)
            self.audit_faster_ws_bytes = int(lib.dd_audit_workspace_bytes_faster(C.byref(params), C.byref(self.audit_faster_view)))
            self.audit_faster_ws = torch.empty(max(self.audit_faster_ws_bytes, 8), dtype=torch.uint8, device=self.device)
        if self.cigars:
            npair = max(pb.n_pairs, 1)
            self.cig = {"n_ops": torch.zeros(npair, dtype=torch.int32, device=self.device),
                        "ops": torch.zeros(npair * self.ops_cap, dtype=torch.int32, device=self.device),    # uint32 bits
                        "ref_off": torch.zeros(npair, dtype=torch.int32, device=self.device),
                        "status": torch.zeros(npair, dtype=torch.int32, device=self.device)}
            self.dcig = capi.dd_cigar_result(*[self.cig[k].data_ptr() for k in ("n_ops", "ops", "ref_off", "status")])

    def launch(self, stream=None):
        """Enqueue the path on `stream` (default: torch's current stream on this device). Asynchronous."""
        if self.long_windows_faster:
            raise RuntimeError("this batch was screened for the --faster model (long_windows_faster=True): use launch_faster()")
        lib = capi.load()
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        if self.wide:                  # no main launch for these parameters: the wide launch writes every pair and every read's onHap
            rc = lib.dd_launch_device_wide(C.byref(self.params), C.byref(self.db), C.byref(self.dr), C.c_void_p(self.long_ws.data_ptr()),
                                           self.long_ws_bytes, C.c_void_p(stream.cuda_stream))
            if rc != 0:
                raise RuntimeError("dd_launch_device_wide rc=%d: %s" % (rc, capi.last_error()))
            return
        rc = lib.dd_launch_device(C.byref(self.params), C.byref(self.db), C.byref(self.dr),
                                  C.c_void_p(self.ws.data_ptr()), self.ws_bytes, C.c_void_p(stream.cuda_stream))
        if rc != 0:
            raise RuntimeError("dd_launch_device rc=%d: %s" % (rc, capi.last_error()))
        if self.n_long:                # after the main launch and its onHap pass, on the same stream
            rc = lib.dd_launch_device_long(C.byref(self.params), C.byref(self.db), C.byref(self.dr), C.c_void_p(self.long_ws.data_ptr()),
                                           self.long_ws_bytes, C.c_void_p(stream.cuda_stream))
            if rc != 0:
                raise RuntimeError("dd_launch_device_long rc=%d: %s" % (rc, capi.last_error()))

    def launch_faster(self, stream=None):
        """The --faster model (ObservationModelS) on the same resident batch. Asynchronous."""
        lib = capi.load()
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        rc = lib.dd_launch_device_faster_ex(C.byref(self.params), C.byref(self.db), C.byref(self.dr), C.c_void_p(stream.cuda_stream), self.opt_wide)
        if rc != 0:
            raise RuntimeError("dd_launch_device_faster_ex rc=%d: %s" % (rc, capi.last_error()))
        if self.long_windows_faster and self.n_long:   # after the main launch and its onHap pass, on the same stream
            rc = lib.dd_launch_device_faster_long(C.byref(self.params), C.byref(self.db), C.byref(self.dr), C.c_void_p(self.long_ws.data_ptr()),
                                                  self.long_ws_bytes, C.c_void_p(stream.cuda_stream))
            if rc != 0:
                raise RuntimeError("dd_launch_device_faster_long rc=%d: %s" % (rc, capi.last_error()))

    def launch_cigars(self, stream=None):
        """The CIGAR of every pair from the hpos of the last launch() / launch_faster() (same stream, behind it). Asynchronous."""
        if not self.cigars:
            raise RuntimeError("this batch was built without cigars=True")
        lib = capi.load()
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        hal = self.t["hap_aligned"].data_ptr() if "hap_aligned" in self.t else None
        rc = lib.dd_cigars_device(C.byref(self.db), C.c_void_p(self.out["hpos"].data_ptr()), C.c_void_p(self.out["status"].data_ptr()),
                                  C.c_void_p(self.t["hap_ref_pos"].data_ptr()), C.c_void_p(hal), C.byref(self.dcig), self.ops_cap,
                                  C.c_void_p(stream.cuda_stream))
        if rc != 0:
            raise RuntimeError("dd_cigars_device rc=%d: %s" % (rc, capi.last_error()))

    def launch_indel_keys(self, stream=None):
        """The --faster model's indel-map key count of every pair, from the hpos and status of the last launch_faster() (same stream,
        behind it). Asynchronous."""
        if not self.indel_keys:
            raise RuntimeError("this batch was built without indel_keys=True")
        lib = capi.load()
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        rc = lib.dd_indel_keys_device(C.byref(self.db), C.c_void_p(self.out["hpos"].data_ptr()), C.c_void_p(self.out["status"].data_ptr()),
                                      C.c_void_p(self.keys.data_ptr()), C.c_void_p(stream.cuda_stream))
        if rc != 0:
            raise RuntimeError("dd_indel_keys_device rc=%d: %s" % (rc, capi.last_error()))

    def launch_audit(self, stream=None):
        """The audit of the sample, from what the last launch() left in the result tensors (same stream, behind it): the long-window
        launch into the shadow tensors, then the comparison into the report. Asynchronous."""
        if self.audit is None:
            raise RuntimeError("this batch was built without audit=N")
        lib = capi.load()
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        rc = lib.dd_audit_device(C.byref(self.params), C.byref(self.db), C.byref(self.dr), C.byref(self.audit_view), C.byref(self.dshadow),
                                 C.c_void_p(self.audit_report_t.data_ptr()), self.audit_max_records, C.c_void_p(self.audit_ws.data_ptr()),
                                 self.audit_ws_bytes, C.c_void_p(stream.cuda_stream))
        if rc != 0:
            raise RuntimeError("dd_audit_device rc=%d: %s" % (rc, capi.last_error()))

    def audit_results(self):
        """Synchronise and copy back the last launch_audit(): capi.audit_report's dict (n_pairs, n_diff, diff and compared per field,
        records) with `shadow`, the shadow arrays trimmed to the sample's lengths, and `sample`, the capi.AuditSample."""
        torch.cuda.synchronize(self.device)
        rep = capi.audit_report(self.audit_report_t.cpu().numpy().view(np.uint8), self.audit_max_records)
        rep["shadow"] = {k: v[:self._shadow_n[k]].cpu().numpy() for k, v in self.shadow.items()}
        rep["sample"] = self.audit
        return rep

    def launch_audit_faster(self, stream=None):
        """The audit of the --faster sample, from what the last launch_faster() left in the result tensors (same stream, behind it): the
        shadow kernel into the shadow tensors, then the comparison into the report. Asynchronous."""
        if self.audit_faster is None:
            raise RuntimeError("this batch was built without audit_faster=N")
        lib = capi.load()
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        rc = lib.dd_audit_device_faster(C.byref(self.params), C.byref(self.db), C.byref(self.dr), C.byref(self.audit_faster_view),
                                        C.byref(self.dshadow_faster), C.c_void_p(self.audit_faster_report_t.data_ptr()), self.audit_max_records,
                                        C.c_void_p(self.audit_faster_ws.data_ptr()), self.audit_faster_ws_bytes, C.c_void_p(stream.cuda_stream))
        if rc != 0:
            raise RuntimeError("dd_audit_device_faster rc=%d: %s" % (rc, capi.last_error()))

    def audit_faster_results(self):
        """Synchronise and copy back the last launch_audit_faster(): audit_results()' dict (n_pairs, n_diff, diff and compared per field,
        records, `shadow`, `sample`)."""
        torch.cuda.synchronize(self.device)
        rep = capi.audit_report(self.audit_faster_report_t.cpu().numpy().view(np.uint8), self.audit_max_records)
        rep["shadow"] = {k: v[:self._shadow_faster_n[k]].cpu().numpy() for k, v in self.shadow_faster.items()}
        rep["sample"] = self.audit_faster
        return rep

    def launch_realign(self, mode, win_hap_pair=None, stream=None, on_hap=True):
        """The haplotype each read is realigned to and that pair's CIGAR, from the ll, onHap, status and hpos of the last launch() /
        launch_faster() (same stream, behind it).  mode: capi.DD_REALIGN_FIRST_MAX, or capi.DD_REALIGN_PAIR with win_hap_pair
        [n_windows, 2] (and hap_n_indels given to the constructor).  on_hap=False: the FIRST_MAX rule without onHap (NULL).
        Asynchronous."""
        if not self.realign:
            raise RuntimeError("this batch was built without realign=True")
        lib = capi.load()
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        pairs = None
        if isinstance(win_hap_pair, torch.Tensor):             # already on the device (launch_diploid_pairs' `pair`): read where it is
            if win_hap_pair.dtype != torch.int32 or win_hap_pair.device != self.device or win_hap_pair.numel() < 2 * self.pb.n_windows:
                raise ValueError("a device win_hap_pair must be an int32 tensor on the batch's device with two entries per window")
            self._win_hap_pair = win_hap_pair
            pairs = win_hap_pair.data_ptr()
        elif win_hap_pair is not None:
            whp = np.ascontiguousarray(win_hap_pair, np.int32).reshape(-1)
            if whp.shape != (2 * self.pb.n_windows,):
                raise ValueError("win_hap_pair must hold two entries per window")
            self._win_hap_pair = _to_dev(whp, self.device)     # the launch reads it: keep it alive
            pairs = self._win_hap_pair.data_ptr()
        hal = self.t["hap_aligned"].data_ptr() if "hap_aligned" in self.t else None
        hni = self.t["hap_n_indels"].data_ptr() if "hap_n_indels" in self.t else None
        rc = lib.dd_realign_device(C.byref(self.db), int(mode), C.c_void_p(self.out["ll"].data_ptr()),
                                   C.c_void_p(self.out["onHap"].data_ptr() if on_hap else None), C.c_void_p(pairs), C.c_void_p(hni),
                                   C.c_void_p(self.out["hpos"].data_ptr()), C.c_void_p(self.out["status"].data_ptr()),
                                   C.c_void_p(self.t["hap_ref_pos"].data_ptr()), C.c_void_p(hal), C.byref(self.drl), self.ops_cap,
                                   C.c_void_p(stream.cuda_stream))
        if rc != 0:
            raise RuntimeError("dd_realign_device rc=%d: %s" % (rc, capi.last_error()))

    def launch_diploid_pairs(self, stream=None):
        """Every window's MAP haplotype pair, chosen and certified from the ll and status of the last launch() (same stream, behind it).
        Asynchronous; returns the device tensors dict(pair [2 * n_windows], state, best, gap, margin)."""
        if self.dip is None:
            raise RuntimeError("this batch was built without diploid_prior")
        lib = capi.load()
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        rc = lib.dd_diploid_pairs_device(C.byref(self.db), C.c_void_p(self.t["win_hh_off"].data_ptr()), C.c_void_p(self.out["ll"].data_ptr()),
                                         C.c_void_p(self.out["status"].data_ptr()), C.c_void_p(self.t["diploid_prior"].data_ptr()),
                                         C.byref(self.ddip), C.c_void_p(stream.cuda_stream))
        if rc != 0:
            raise RuntimeError("dd_diploid_pairs_device rc=%d: %s" % (rc, capi.last_error()))
        return self.dip

    def diploid_pair_results(self):
        """Synchronise and copy back the outputs of the last launch_diploid_pairs(): dict(pair [n_windows, 2], state, best, gap, margin)."""
        torch.cuda.synchronize(self.device)
        n = self.pb.n_windows
        res = {k: self.dip[k][:n * (2 if k == "pair" else 1)].cpu().numpy() for k in capi.DIPLOID_PAIR_FIELDS}
        res["pair"] = res["pair"].reshape(n, 2)
        return res

    def pooled_em(self, slots, a0=0.001, tol=1e-4, stream=None):
        """The pooled analysis' EM loop (dd_pooled_em_device) on the `ll` of the last launch() / launch_faster(), resident in HBM (same
        stream, behind it).  slots: pooled.pack_slots(...).  Asynchronous; returns the device tensors dict(loglik, freqs, iters, ediff),
        which pooled_em_results() copies back."""
        lib = capi.load()
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        nh = np.diff(self.pb.a["win_hap_off"])
        n, f = len(slots["slot_window"]), int(slots["slot_off"][-1])
        t_in = {k: _to_dev(slots[k], self.device) for k in ("slot_window", "slot_off", "compat")}
        out = {"loglik": torch.zeros(max(n, 1), dtype=torch.float64, device=self.device),
               "freqs": torch.zeros(max(f, 1), dtype=torch.float64, device=self.device),
               "iters": torch.zeros(max(n, 1), dtype=torch.int32, device=self.device),
               "ediff": torch.zeros(max(n, 1), dtype=torch.float64, device=self.device)}
        s = capi.dd_pooled_slots(n, *[t_in[k].data_ptr() for k in ("slot_window", "slot_off", "compat")])
        r = capi.dd_pooled_result(*[out[k].data_ptr() for k in capi.POOLED_RESULT_FIELDS])
        rc = lib.dd_pooled_em_device(C.byref(self.db), C.c_void_p(self.out["ll"].data_ptr()), C.byref(s), int(nh.max()) if len(nh) else 0,
                                     a0, tol, C.byref(r), C.c_void_p(stream.cuda_stream))
        if rc != 0:
            raise RuntimeError("dd_pooled_em_device rc=%d: %s" % (rc, capi.last_error()))
        self._pooled = (t_in, out, n, f)       # the launch reads and writes these: keep them alive
        return out

    def pooled_em_results(self):
        """Synchronise and copy back the outputs of the last pooled_em(): dict(loglik, freqs, iters, ediff) as pooled.em returns them."""
        torch.cuda.synchronize(self.device)
        _, out, n, f = self._pooled
        return {k: out[k][:(f if k == "freqs" else n)].cpu().numpy() for k in capi.POOLED_RESULT_FIELDS}

    def results(self):
        """Host copies (numpy) of the outputs, trimmed to their logical lengths."""
        torch.cuda.synchronize(self.device)
        res = {k: self.out[k][:self._n[k]].cpu().numpy() for k, _ in capi.RESULT_FIELDS}
        if self.cigars:
            n = self.pb.n_pairs
            for k in ("n_ops", "ref_off", "status"):
                res["cigar_" + k] = self.cig[k][:n].cpu().numpy()
            res["cigar_ops"] = self.cig["ops"][:n * self.ops_cap].cpu().numpy().view(np.uint32).reshape(n, self.ops_cap)
        if self.indel_keys:
            res["indel_keys"] = self.keys[:self.pb.n_pairs].cpu().numpy()
        if self.realign:
            n = self.pb.n_reads
            for k in ("hap", "status", "n_ops", "ref_off"):
                res["realign_" + k] = self.rl[k][:n].cpu().numpy()
            res["realign_ops"] = self.rl["ops"][:n * self.ops_cap].cpu().numpy().view(np.uint32).reshape(n, self.ops_cap)
        return res
