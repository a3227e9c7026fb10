"""ctypes binding of the C ABI in include/dindel_hmm.h (libdindel_hmm.so).

This is the test/bench harness' way into the product library — the same symbols a C++ host (the
reference's DetInDel::computeLikelihoods, DInDel.cpp:1707-1739) binds directly.  There is no Python
or CPU implementation behind it: if the shared library is missing, loading raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DD_LIB_PATH: A/B a diagnostic build of the SAME library (tools/); never a different implementation
LIB_PATH = os.environ.get("DD_LIB_PATH") or os.path.join(_HERE, "csrc", "libdindel_hmm.so")

c_i32p = C.POINTER(C.c_int32)
c_i64p = C.POINTER(C.c_int64)
c_u32p = C.POINTER(C.c_uint32)
c_u8p = C.POINTER(C.c_uint8)
c_i16p = C.POINTER(C.c_int16)
c_f64p = C.POINTER(C.c_double)

DD_TABLE_DOUBLES = 32 + 4 * 256 + 4 * 256 + 2 * 64 + 2 * 256 + 2 * 256 + 64
DD_READ_UNMAPPED, DD_READ_PAIRED, DD_READ_MATE_UNMAPPED, DD_READ_MATE_REVERSE, DD_READ_MATE_SAME_TID = 1, 2, 4, 8, 16

ABI_VERSION = 13           # DD_ABI_VERSION of include/dindel_hmm.h
DD_HPOS_INS, DD_HPOS_LO, DD_HPOS_RO, DD_HPOS_INS_KEY0 = -1, -3, -4, -16

DD_SUCCESS, DD_ERR_NO_DEVICE, DD_ERR_INVALID, DD_ERR_UNSUPPORTED, DD_ERR_HIP = 0, -1, -2, -3, -4
DD_PAIR_OK, DD_PAIR_HAPSIZE, DD_PAIR_NAN, DD_PAIR_LLPOS, DD_PAIR_UNSUPPORTED = 0, 1, 2, 3, 4
DD_MAX_HAP_LEN, DD_MAX_READ_LEN = 766, 1024
DD_LONG_MAX_HAP_LEN, DD_LONG_MAX_READ_LEN = 4094, 4096      # the long-window path (opt-in)
DD_OPT_LONG_WINDOWS = 1
DD_OPT_LONG_WINDOWS_FASTER = 2     # the --faster model's own long-window option
DD_OPT_WIDE_DELETIONS = 4          # maxLengthDel above 31: the long-window kernel's wide build (with DD_OPT_LONG_WINDOWS)
DD_MAX_LENGTH_DEL = 31
DD_WIDE_MAX_LENGTH_DEL = 2 ** 31 - 3
DD_LONG_LOG_WIDE = 256             # added to a long launch record's K when the wide build ran
DD_FASTER_LONG_WS_BUDGET = 512 << 20
DD_WIN_MAIN, DD_WIN_UNSUPPORTED, DD_WIN_LONG = 0, 1, 2
DD_LONG_WS_BUDGET = 512 << 20
# device-side getCIGAR (opt-in): per-pair status codes, in the order of host/cigar.cpp's throw strings
(DD_CIGAR_OK, DD_CIGAR_HAP_NOT_ALIGNED, DD_CIGAR_ERROR1, DD_CIGAR_ERROR2, DD_CIGAR_ERROR3, DD_CIGAR_ERROR4, DD_CIGAR_IMPOSSIBLE,
 DD_CIGAR_OVERFLOW, DD_CIGAR_NOT_COMPUTED) = range(9)
DD_CIGAR_DEFAULT_OPS_CAP = 8
# realigned reads (opt-in): per-read status codes beside the DD_CIGAR_* of the chosen pair, and the two rules
DD_REALIGN_OFF_HAP, DD_REALIGN_BAD_PAIR, DD_REALIGN_NO_HAPS = 9, 10, 11
DD_REALIGN_FIRST_MAX, DD_REALIGN_PAIR = 0, 1
# the certified MAP haplotype pair of the diploid realigned reads (opt-in): per-window states and the haplotype cap
(DD_DIPPAIR_CERTIFIED, DD_DIPPAIR_TIE, DD_DIPPAIR_NONFINITE, DD_DIPPAIR_NOT_COMPUTED, DD_DIPPAIR_NO_HAPS, DD_DIPPAIR_TOO_MANY_HAPS) = range(6)
DD_DIPPAIR_MAX_HAPS = 128
# the --faster model's indel-map key count (opt-in): one int16 per pair, the count or one of the two negative marks
DD_INDEL_KEYS_CAP, DD_INDEL_KEYS_OVERFLOW, DD_INDEL_KEYS_NOT_COMPUTED = 64, -1, -2
# audit (opt-in): the field ids of a difference record, in dd_result's comparison order, and the record of the audit's long launch
AUDIT_FIELDS = ["status", "ll", "llOn", "llOff", "mLogBQ", "offHap", "offHapHMQ", "numIndels", "numMismatch", "nBQT", "nmmBQT", "nMMLeft",
                "nMMRight", "firstBase", "lastBase", "hpos", "var_covered", "var_fcov"]
DD_AUDIT_N_FIELDS = len(AUDIT_FIELDS)
AUDIT_LOG_FIELDS = ["grid", "pairs", "max_pairs_per_wg", "ws_bytes", "K", "max_hap", "max_read", "compare_grid"]
AUDIT_FASTER_LOG_FIELDS = ["grid", "pairs", "in_lds", "ws_bytes", "lds_bytes", "max_hap", "max_read", "compare_grid"]   # dd_audit_last_launch_faster
# alignHaplotypes on the device: per-pair status codes and the launch geometry record
DD_ALIGN_OK, DD_ALIGN_EMPTY, DD_ALIGN_TOO_LONG, DD_ALIGN_BAD_REF = range(4)
DD_ALIGN_WS_BUDGET = 512 << 20
ALIGN_LOG_FIELDS = ["grid", "waves", "tile_bytes", "lds_block", "pairs", "ws_bytes", "max_draws", "guard_trips"]
# the indel events of an alignment (dd_align_events records)
DD_ALIGN_EVENT_INS, DD_ALIGN_EVENT_DEL = 1, 2
DD_ALIGN_EVENTS_MAX_CAP = 4096
ALIGN_EVENTS_LOG_FIELDS = ["grid", "pairs", "max_draws", "guard_trips"]
# the variants of an alignment (dd_hap_variant records, dd_hap_variants_summary); the launch record has ALIGN_EVENTS_LOG_FIELDS
DD_HAP_VARIANT_SNP, DD_HAP_VARIANT_DEL_UNSEEN = 3, 4
DD_HAP_VARIANTS_LO_FIRST, DD_HAP_VARIANTS_RO_LAST, DD_HAP_VARIANTS_HOST = 1, 2, 4
DD_HAP_VARIANTS_MAX_CAP = 4096
# the block table of a window's haplotype distribution: per-window status codes, limits and the launch record
DD_HAPDIST_OK, DD_HAPDIST_TOO_WIDE, DD_HAPDIST_OVERFLOW, DD_HAPDIST_HOST = range(4)
DD_HAPDIST_MAX_WINDOW, DD_HAPDIST_MAX_DISTINCT, DD_HAPDIST_MAX_INS_POS = 1024, 16, 64
HAP_BLOCKS_LOG_FIELDS = ["grid", "windows", "max_draws", "guard_trips"]
CIGAR_MESSAGES = {DD_CIGAR_HAP_NOT_ALIGNED: "Haplotype has not been aligned!", DD_CIGAR_ERROR1: "Error(1)!", DD_CIGAR_ERROR2: "Error(2)!",
                  DD_CIGAR_ERROR3: "Error(3)!", DD_CIGAR_ERROR4: "Error(4)!", DD_CIGAR_IMPOSSIBLE: "How is this possible? (1)"}


class dd_params(C.Structure):
    _fields_ = [("pError", C.c_double), ("pMut", C.c_double), ("pFirstgLO", C.c_double),
                ("mapQualThreshold", C.c_double), ("checkBaseQualThreshold", C.c_double),
                ("maxLengthDel", C.c_int32), ("padCover", C.c_int32), ("bMid", C.c_int32),
                ("forceReadOnHaplotype", C.c_int32), ("mapUnmappedReads", C.c_int32), ("maxMismatch", C.c_int32), ("capMapQualFast", C.c_double)]

    @classmethod
    def from_dict(cls, d):
        p = cls()
        for k, v in d.items():
            setattr(p, k, v)
        return p

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def params_cli_defaults():
    """DInDel.cpp:3937-3949 + 4122-4157 (the set production runs use)."""
    return dd_params(5e-4, 1e-5, 0.01, 100.0, 0.95, 5, 2, -1, 0, 0, 2, 45.0)


def params_struct_defaults():
    """ObservationModel.hpp:39-64."""
    return dd_params(1e-4, 1e-4, 0.01, 100.0, 0.95, 10, 5, -1, 0, 0, 1, 40.0)


class dd_batch(C.Structure):
    _fields_ = [("n_windows", C.c_int32),
                ("win_hap_off", c_i32p), ("win_read_off", c_i32p), ("win_hap_start", c_u32p),
                ("hap_seq_off", c_i32p), ("hap_seq", C.c_char_p), ("hap_var_off", c_i32p), ("hap_var", c_i32p),
                ("read_seq_off", c_i32p), ("read_seq", C.c_char_p), ("read_qidx", c_u8p), ("read_mqidx", c_u8p),
                ("read_start", c_u32p), ("read_flags", c_u8p),
                ("n_qual", C.c_int32), ("qual_table", c_f64p),
                ("n_mapq", C.c_int32), ("mapq_table", c_f64p), ("hap_var_flank", c_i32p),
                ("read_mate_pos", c_i32p), ("read_mate_len", c_i32p), ("read_lib", c_u8p),
                ("n_libs", C.c_int32), ("lib_off", c_i32p), ("lib_prob", c_f64p), ("lib_p95", c_f64p)]


RESULT_FIELDS = [("ll", c_f64p), ("llOn", c_f64p), ("llOff", c_f64p), ("mLogBQ", c_f64p),
                 ("offHap", c_u8p), ("offHapHMQ", c_u8p),
                 ("numIndels", c_i16p), ("numMismatch", c_i16p), ("nBQT", c_i16p), ("nmmBQT", c_i16p),
                 ("nMMLeft", c_i16p), ("nMMRight", c_i16p), ("firstBase", c_i16p), ("lastBase", c_i16p),
                 ("hpos", c_i16p), ("var_covered", c_u8p), ("status", c_i32p), ("onHap", c_u8p), ("var_fcov", c_u8p)]


class dd_result(C.Structure):
    _fields_ = RESULT_FIELDS


class dd_sizes(C.Structure):
    _fields_ = [("n_haps", C.c_int64), ("n_reads", C.c_int64), ("n_pairs", C.c_int64),
                ("hap_bases", C.c_int64), ("read_bases", C.c_int64), ("hpos_len", C.c_int64),
                ("var_cov_len", C.c_int64), ("cells", C.c_int64),
                ("max_hap_len", C.c_int32), ("max_read_len", C.c_int32)]


class dd_device_batch(C.Structure):
    _fields_ = [("n_windows", C.c_int32), ("n_haps", C.c_int32), ("n_reads", C.c_int32),
                ("max_hap_len", C.c_int32), ("max_read_len", C.c_int32), ("max_window_reads", C.c_int32),
                ("win_hap_off", C.c_void_p), ("win_read_off", C.c_void_p), ("win_hap_start", C.c_void_p),
                ("hap_seq_off", C.c_void_p), ("hap_seq", C.c_void_p), ("hap_var_off", C.c_void_p), ("hap_var", C.c_void_p),
                ("read_seq_off", C.c_void_p), ("read_seq", C.c_void_p), ("read_qidx", C.c_void_p), ("read_mqidx", C.c_void_p),
                ("read_start", C.c_void_p), ("read_flags", C.c_void_p),
                ("hap_window", C.c_void_p), ("win_pair_off", C.c_void_p), ("win_hpos_off", C.c_void_p),
                ("win_varcov_off", C.c_void_p), ("tables", C.c_void_p),
                ("n_qual", C.c_int32), ("n_mapq", C.c_int32), ("hap_var_flank", C.c_void_p), ("sym_lut", C.c_void_p),
                ("read_mate_pos", C.c_void_p), ("read_mate_len", C.c_void_p), ("read_lib", C.c_void_p),
                ("lib_off", C.c_void_p), ("lib_logprob", C.c_void_p), ("lib_log95", C.c_void_p),
                ("hap_class_list", C.c_void_p), ("classes", C.c_void_p), ("win_skip", C.c_void_p),
                ("long_max_hap_len", C.c_int32), ("long_max_read_len", C.c_int32)]


# haplotype-length classes of a ragged batch, one per lane tiling (plan.cpp kHapClasses): longest haplotype, pairs per wavefront, positions per lane
HAP_CLASSES = [(30, 2, 1), (62, 1, 1), (94, 2, 3), (126, 1, 2), (158, 2, 5), (190, 1, 3), (222, 1, 4), (254, 1, 4), (318, 1, 5), (382, 1, 6),
               (446, 1, 7), (510, 1, 8), (574, 1, 9), (638, 1, 10), (702, 1, 11), (766, 1, 12)]
HAP_CLASS_BOUNDS = [c[0] for c in HAP_CLASSES]


N_HAP_CLASSES, N_READ_CLASSES = 16, 3


class dd_launch_class(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("list_off", "list_len", "hap_class", "max_hap_len", "min_read_len", "max_read_len",
                                         "max_window_reads", "avg_window_reads", "avg_read_len")]


class dd_length_classes(C.Structure):
    _fields_ = [("n_launches", C.c_int32), ("list_len", C.c_int32), ("launch", dd_launch_class * (N_HAP_CLASSES * N_READ_CLASSES))]


class dd_cigar_result(C.Structure):
    """Per pair: n_ops (int32), ops (uint32 [ops_cap]), ref_off (int32), status (int32).  Raw addresses: host arrays for
    dd_compute_likelihoods_cigars, device arrays for dd_cigars_device."""
    _fields_ = [("n_ops", C.c_void_p), ("ops", C.c_void_p), ("ref_off", C.c_void_p), ("status", C.c_void_p)]


REALIGN_RESULT_FIELDS = ("hap", "status", "n_ops", "ops", "ref_off")


class dd_realign_result(C.Structure):
    """Per read: hap, status, n_ops (int32), ops (uint32 [ops_cap]), ref_off (int32).  Raw addresses: host arrays for
    dd_compute_likelihoods_realign, device arrays for dd_realign_device."""
    _fields_ = [(n, C.c_void_p) for n in REALIGN_RESULT_FIELDS]


DIPLOID_PAIR_FIELDS = ("pair", "state", "best", "gap", "margin")
DIPLOID_PAIR_DTYPES = {"pair": "int32", "state": "int32", "best": "float64", "gap": "float64", "margin": "float64"}


class dd_diploid_pair_result(C.Structure):
    """Per window: pair (int32 [2]), state (int32, DD_DIPPAIR_*), best, gap, margin (double).  Raw addresses: host arrays for
    dd_diploid_pairs_host, device arrays for dd_diploid_pairs_device."""
    _fields_ = [(n, C.c_void_p) for n in DIPLOID_PAIR_FIELDS]


class dd_align_batch(C.Structure):
    """References and the haplotypes aligned against them.  Raw addresses: host arrays for dd_align_haplotypes and
    dd_align_workspace_bytes, device arrays for dd_align_haplotypes_device."""
    _fields_ = [("n_refs", C.c_int32), ("ref_off", C.c_void_p), ("ref_seq", C.c_void_p), ("n_pairs", C.c_int32), ("pair_ref", C.c_void_p),
                ("hap_off", C.c_void_p), ("hap_seq", C.c_void_p)]


class dd_align_result(C.Structure):
    """score, status (int32 [n_pairs]) and ref_pos (int16, laid out like hap_seq); raw addresses like dd_align_batch."""
    _fields_ = [("score", C.c_void_p), ("status", C.c_void_p), ("ref_pos", C.c_void_p)]


class dd_align_events(C.Structure):
    """One indel of one pair as convertAlignment keys it: kind (DD_ALIGN_EVENT_*), ref, len, hap."""
    _fields_ = [("kind", C.c_int16), ("ref", C.c_int16), ("len", C.c_int16), ("hap", C.c_int16)]


class dd_hap_variant(C.Structure):
    """One variant of one pair with the four values of setFlanking: kind (DD_ALIGN_EVENT_INS / _DEL, DD_HAP_VARIANT_*), key, len, start_read."""
    _fields_ = [(n, C.c_int16) for n in ("kind", "key", "len", "start_read", "left_flank_hap", "right_flank_hap", "left_flank_read", "right_flank_read")]


class dd_hap_variants_summary(C.Structure):
    """Per pair: the true record count, ml.firstBase / ml.lastBase and DD_HAP_VARIANTS_* flags."""
    _fields_ = [(n, C.c_int32) for n in ("n_variants", "first_base", "last_base", "flags")]


class dd_hap_batch(C.Structure):
    """Windows and the reads laid over them (block table of the haplotype distribution).  Raw addresses: host arrays for
    dd_hap_blocks_compute and dd_hap_blocks_offsets, device arrays for dd_hap_blocks_device."""
    _fields_ = [("n_windows", C.c_int32), ("win_rs", C.c_void_p), ("win_ref_off", C.c_void_p), ("ref_seq", C.c_void_p),
                ("win_read_off", C.c_void_p), ("n_reads", C.c_int32), ("read_pos", C.c_void_p), ("read_flag", C.c_void_p),
                ("read_op_off", C.c_void_p), ("ops", C.c_void_p), ("read_base_off", C.c_void_p), ("bases", C.c_void_p)]


HAP_BLOCKS_WINDOW_FIELDS = ("status", "n_blocks", "n_entries", "n_ins_ops", "n_ins_pos", "left")
HAP_BLOCKS_OFFSET_FIELDS = ("blk_off", "ent_off", "ins_off")
HAP_BLOCKS_TABLE_FIELDS = ("blocks", "entries", "ins_ops", "ins_pos")


class dd_hap_blocks(C.Structure):
    """The block tables of a dd_hap_batch; raw addresses like dd_hap_batch."""
    _fields_ = [(n, C.c_void_p) for n in HAP_BLOCKS_WINDOW_FIELDS + HAP_BLOCKS_OFFSET_FIELDS + HAP_BLOCKS_TABLE_FIELDS]


class dd_pooled_slots(C.Structure):
    """Slots of the pooled analysis' EM loop: slot_window (int32 [n_slots]), slot_off (int64 [n_slots + 1]), compat (uint8).  Raw addresses:
    host arrays for dd_pooled_em and dd_pooled_em_host, device arrays for dd_pooled_em_device."""
    _fields_ = [("n_slots", C.c_int64), ("slot_window", C.c_void_p), ("slot_off", C.c_void_p), ("compat", C.c_void_p)]


POOLED_RESULT_FIELDS = ("loglik", "freqs", "iters", "ediff")
DD_POOLED_MAX_HAPS = 256


class dd_pooled_result(C.Structure):
    """loglik, ediff (double [n_slots]), iters (int32 [n_slots]), freqs (double, laid out like compat); raw addresses like dd_pooled_slots."""
    _fields_ = [(n, C.c_void_p) for n in POOLED_RESULT_FIELDS]


class dd_audit_record(C.Structure):
    """One difference of an audit: window, field (index into AUDIT_FIELDS), pair, the element's index in the primary array, both values'
    bits zero-extended."""
    _fields_ = [("window", C.c_int32), ("field", C.c_int32), ("pair", C.c_int64), ("index", C.c_int64),
                ("primary_bits", C.c_uint64), ("shadow_bits", C.c_uint64)]


class dd_audit_report(C.Structure):
    """The header of an audit's report; max_records dd_audit_record follow it."""
    _fields_ = [("n_pairs", C.c_int64), ("n_diff", C.c_int64), ("diff", C.c_int64 * DD_AUDIT_N_FIELDS), ("compared", C.c_int64 * DD_AUDIT_N_FIELDS)]


class dd_audit_sizes(C.Structure):
    _fields_ = [("n_windows", C.c_int32), ("max_hap_len", C.c_int32), ("max_read_len", C.c_int32), ("reserved", C.c_int32),
                ("n_pairs", C.c_int64), ("hpos_len", C.c_int64), ("var_cov_len", C.c_int64)]


class dd_audit_view(C.Structure):
    """dd_audit_select's outputs where the comparison runs.  Raw addresses: device arrays for dd_audit_device, host arrays for
    dd_audit_compare_host."""
    _fields_ = [("n_windows", C.c_int32), ("n_qual", C.c_int32), ("audit_class", C.c_void_p), ("pair_off", C.c_void_p), ("hpos_off", C.c_void_p),
                ("varcov_off", C.c_void_p), ("sizes", dd_audit_sizes)]


class dd_device_result(C.Structure):
    """dd_result with raw device addresses (same layout: every member is a pointer)."""
    _fields_ = [(n, C.c_void_p) for n, _ in RESULT_FIELDS]


EXPORTS = ["dd_params_struct_defaults", "dd_params_cli_defaults", "dd_batch_sizes", "dd_batch_offsets", "dd_screen_windows",
           "dd_compute_likelihoods", "dd_compute_likelihoods_faster", "dd_compute_likelihoods_multi", "dd_compute_likelihoods_faster_multi", "dd_partition_windows", "dd_launch_device_faster", "dd_release_cache", "dd_reserve_cache", "dd_host_alloc", "dd_host_free", "dd_build_tables", "dd_build_symbol_lut", "dd_build_library_tables", "dd_build_length_classes", "dd_plan_info", "dd_build_index", "dd_workspace_bytes",
           "dd_launch_device", "dd_kernel_name", "dd_last_launch", "dd_launch_log", "dd_last_direct_outputs", "dd_pair_sum_offsets", "dd_pair_sums_device",
           "dd_pair_sums", "dd_map_pairs_device", "dd_map_pairs", "dd_last_error", "dd_abi_version", "dd_device_count",
           "dd_screen_windows_ex", "dd_compute_likelihoods_ex", "dd_workspace_bytes_long", "dd_launch_device_long", "dd_long_launch_log",
           "dd_compute_likelihoods_faster_ex", "dd_workspace_bytes_faster_long", "dd_launch_device_faster_long", "dd_faster_long_launch_log",
           "dd_cigars_device", "dd_compute_likelihoods_cigars", "dd_realign_device", "dd_compute_likelihoods_realign",
           "dd_align_haplotypes", "dd_align_workspace_bytes", "dd_align_haplotypes_device", "dd_align_last_launch",
           "dd_align_events_device", "dd_align_haplotypes_events", "dd_align_events_last_launch",
           "dd_hap_variants_device", "dd_align_haplotypes_variants", "dd_hap_variants_last_launch",
           "dd_hap_blocks_offsets", "dd_hap_blocks_workspace_bytes", "dd_hap_blocks_device", "dd_hap_blocks_compute", "dd_hap_blocks_last_launch",
           "dd_pooled_em_device", "dd_pooled_em", "dd_pooled_em_host", "dd_pooled_math_eval",
           "dd_diploid_pairs_device", "dd_diploid_pairs_host", "dd_compute_likelihoods_realign_diploid",
           "dd_indel_keys_device", "dd_indel_keys_host", "dd_compute_likelihoods_faster_keys",
           "dd_audit_select", "dd_audit_workspace_bytes", "dd_audit_device", "dd_audit_last_launch", "dd_audit_compare_host",
           "dd_compute_likelihoods_audit", "dd_audit_inject_next",
           "dd_audit_select_faster", "dd_audit_workspace_bytes_faster", "dd_audit_device_faster", "dd_audit_last_launch_faster",
           "dd_audit_shadow_faster_host", "dd_audit_compare_host_faster", "dd_compute_likelihoods_faster_audit",
           "dd_build_tables_ex", "dd_workspace_bytes_wide", "dd_launch_device_wide", "dd_launch_device_faster_ex"]

_lib = None


def load():
    """Load libdindel_hmm.so; raises (loudly) when the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback for the likelihood path)" % LIB_PATH)
    # One HIP runtime per process: torch bundles its own libamdhip64 (SONAME libamdhip64.so.7).  Load it
    # FIRST so that our NEEDED libamdhip64.so.7 binds to the same copy; otherwise device pointers and
    # streams handed over from torch belong to a different runtime instance.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    lib.dd_params_struct_defaults.argtypes = [C.POINTER(dd_params)]
    lib.dd_params_struct_defaults.restype = None
    lib.dd_params_cli_defaults.argtypes = [C.POINTER(dd_params)]
    lib.dd_params_cli_defaults.restype = None
    lib.dd_batch_sizes.argtypes = [C.POINTER(dd_batch), C.POINTER(dd_sizes)]
    lib.dd_batch_offsets.argtypes = [C.POINTER(dd_batch), c_i64p, c_i64p, c_i64p]
    lib.dd_compute_likelihoods.argtypes = [C.POINTER(dd_params), C.POINTER(dd_batch), C.POINTER(dd_result), C.c_int]
    lib.dd_compute_likelihoods_faster.argtypes = [C.POINTER(dd_params), C.POINTER(dd_batch), C.POINTER(dd_result), C.c_int]
    lib.dd_compute_likelihoods_multi.argtypes = [C.POINTER(dd_params), C.POINTER(dd_batch), C.POINTER(dd_result), c_i32p, C.c_int]
    lib.dd_compute_likelihoods_faster_multi.argtypes = lib.dd_compute_likelihoods_multi.argtypes
    lib.dd_partition_windows.argtypes = [C.POINTER(dd_batch), C.c_int, c_i32p]
    lib.dd_launch_device_faster.argtypes = [C.POINTER(dd_params), C.POINTER(dd_device_batch), C.POINTER(dd_device_result), C.c_void_p]
    lib.dd_release_cache.restype = None
    lib.dd_host_alloc.argtypes = [C.c_size_t]
    lib.dd_host_alloc.restype = C.c_void_p
    lib.dd_host_free.argtypes = [C.c_void_p]
    lib.dd_host_free.restype = None
    lib.dd_build_tables.argtypes = [C.POINTER(dd_params), c_f64p, C.c_int, c_f64p, C.c_int, c_f64p]
    lib.dd_build_symbol_lut.argtypes = [C.POINTER(dd_batch), C.POINTER(C.c_uint8)]
    lib.dd_build_library_tables.argtypes = [C.POINTER(dd_batch), c_f64p, c_f64p]
    lib.dd_build_length_classes.argtypes = [C.POINTER(dd_batch), c_u8p, C.POINTER(dd_params), c_i32p, C.POINTER(dd_length_classes)]
    lib.dd_screen_windows.argtypes = [C.POINTER(dd_batch), c_u8p, C.POINTER(C.c_int32 * 2)]
    lib.dd_plan_info.argtypes = [C.POINTER(dd_params), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32 * 10)]
    lib.dd_build_index.argtypes = [C.POINTER(dd_batch), c_i32p, c_i64p, c_i64p, c_i64p]
    lib.dd_workspace_bytes.argtypes = [C.POINTER(dd_params), C.POINTER(dd_device_batch)]
    lib.dd_workspace_bytes.restype = C.c_size_t
    lib.dd_launch_device.argtypes = [C.POINTER(dd_params), C.POINTER(dd_device_batch), C.POINTER(dd_device_result),
                                     C.c_void_p, C.c_size_t, C.c_void_p]
    lib.dd_pair_sum_offsets.argtypes = [C.POINTER(dd_batch), c_i64p]
    lib.dd_pair_sums_device.argtypes = [C.POINTER(dd_device_batch), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.dd_pair_sums.argtypes = [C.POINTER(dd_batch), c_f64p, c_f64p, C.c_int]
    lib.dd_map_pairs_device.argtypes = [C.POINTER(dd_device_batch)] + [C.c_void_p] * 9
    lib.dd_map_pairs.argtypes = [C.POINTER(dd_batch), c_f64p, c_f64p, C.POINTER(C.c_uint8), c_i32p, c_f64p, c_f64p, c_i32p, c_f64p, C.c_int]
    lib.dd_screen_windows_ex.argtypes = [C.POINTER(dd_params), C.POINTER(dd_batch), C.c_uint32, c_u8p, C.POINTER(C.c_int32 * 4)]
    lib.dd_compute_likelihoods_ex.argtypes = [C.POINTER(dd_params), C.POINTER(dd_batch), C.POINTER(dd_result), C.c_int, C.c_uint32]
    lib.dd_workspace_bytes_long.argtypes = [C.POINTER(dd_params), C.POINTER(dd_device_batch)]
    lib.dd_workspace_bytes_long.restype = C.c_size_t
    lib.dd_launch_device_long.argtypes = [C.POINTER(dd_params), C.POINTER(dd_device_batch), C.POINTER(dd_device_result),
                                          C.c_void_p, C.c_size_t, C.c_void_p]
    lib.dd_long_launch_log.argtypes = [c_i64p, C.c_int]
    lib.dd_build_tables_ex.argtypes = lib.dd_build_tables.argtypes + [C.c_uint32]
    lib.dd_workspace_bytes_wide.argtypes = lib.dd_workspace_bytes_long.argtypes
    lib.dd_workspace_bytes_wide.restype = C.c_size_t
    lib.dd_launch_device_wide.argtypes = lib.dd_launch_device_long.argtypes
    lib.dd_launch_device_faster_ex.argtypes = lib.dd_launch_device_faster.argtypes + [C.c_uint32]
    lib.dd_compute_likelihoods_faster_ex.argtypes = lib.dd_compute_likelihoods_ex.argtypes
    lib.dd_workspace_bytes_faster_long.argtypes = [C.POINTER(dd_params), C.POINTER(dd_device_batch)]
    lib.dd_workspace_bytes_faster_long.restype = C.c_size_t
    lib.dd_launch_device_faster_long.argtypes = lib.dd_launch_device_long.argtypes
    lib.dd_faster_long_launch_log.argtypes = [c_i64p, C.c_int]
    lib.dd_cigars_device.argtypes = [C.POINTER(dd_device_batch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(dd_cigar_result),
                                     C.c_int, C.c_void_p]
    lib.dd_compute_likelihoods_cigars.argtypes = [C.POINTER(dd_params), C.POINTER(dd_batch), C.POINTER(dd_result), c_i32p, c_u8p,
                                                  C.POINTER(dd_cigar_result), C.c_int, C.c_int, C.c_uint32]
    lib.dd_realign_device.argtypes = [C.POINTER(dd_device_batch), C.c_int] + [C.c_void_p] * 8 + [C.POINTER(dd_realign_result), C.c_int, C.c_void_p]
    lib.dd_compute_likelihoods_realign.argtypes = [C.POINTER(dd_params), C.POINTER(dd_batch), C.POINTER(dd_result), C.c_int, c_i32p, c_i32p,
                                                   c_i32p, c_u8p, C.POINTER(dd_realign_result), C.c_int, C.c_int, C.c_uint32]
    lib.dd_align_haplotypes.argtypes = [C.POINTER(dd_align_batch), C.POINTER(dd_align_result), C.c_int]
    lib.dd_align_workspace_bytes.argtypes = [C.POINTER(dd_align_batch)]
    lib.dd_align_workspace_bytes.restype = C.c_size_t
    lib.dd_align_haplotypes_device.argtypes = [C.POINTER(dd_align_batch), C.POINTER(dd_align_result), C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                               C.c_void_p]
    lib.dd_align_last_launch.argtypes = [C.POINTER(C.c_int64 * len(ALIGN_LOG_FIELDS))]
    lib.dd_align_last_launch.restype = None
    lib.dd_align_events_device.argtypes = [C.POINTER(dd_align_batch), C.POINTER(dd_align_result), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.dd_align_haplotypes_events.argtypes = [C.POINTER(dd_align_batch), C.POINTER(dd_align_result), C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.dd_align_events_last_launch.argtypes = [C.POINTER(C.c_int64 * len(ALIGN_EVENTS_LOG_FIELDS))]
    lib.dd_align_events_last_launch.restype = None
    lib.dd_hap_variants_device.argtypes = [C.POINTER(dd_align_batch), C.POINTER(dd_align_result), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.dd_align_haplotypes_variants.argtypes = [C.POINTER(dd_align_batch), C.POINTER(dd_align_result), C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.dd_hap_variants_last_launch.argtypes = [C.POINTER(C.c_int64 * len(ALIGN_EVENTS_LOG_FIELDS))]
    lib.dd_hap_variants_last_launch.restype = None
    lib.dd_hap_blocks_offsets.argtypes = [C.POINTER(dd_hap_batch), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.dd_hap_blocks_workspace_bytes.argtypes = []
    lib.dd_hap_blocks_workspace_bytes.restype = C.c_size_t
    lib.dd_hap_blocks_device.argtypes = [C.POINTER(dd_hap_batch), C.POINTER(dd_hap_blocks), C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t,
                                         C.c_void_p]
    lib.dd_hap_blocks_compute.argtypes = [C.POINTER(dd_hap_batch), C.POINTER(dd_hap_blocks), C.c_int]
    lib.dd_hap_blocks_last_launch.argtypes = [C.POINTER(C.c_int64 * len(HAP_BLOCKS_LOG_FIELDS))]
    lib.dd_hap_blocks_last_launch.restype = None
    lib.dd_pooled_em_device.argtypes = [C.POINTER(dd_device_batch), C.c_void_p, C.POINTER(dd_pooled_slots), C.c_int, C.c_double, C.c_double,
                                        C.POINTER(dd_pooled_result), C.c_void_p]
    lib.dd_pooled_em.argtypes = [C.POINTER(dd_batch), c_f64p, C.POINTER(dd_pooled_slots), C.c_double, C.c_double, C.POINTER(dd_pooled_result), C.c_int]
    lib.dd_pooled_em_host.argtypes = lib.dd_pooled_em.argtypes
    lib.dd_pooled_math_eval.argtypes = [C.c_int, c_f64p, c_f64p, C.c_int64]
    lib.dd_diploid_pairs_device.argtypes = [C.POINTER(dd_device_batch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.POINTER(dd_diploid_pair_result), C.c_void_p]
    lib.dd_diploid_pairs_host.argtypes = [C.POINTER(dd_batch), c_f64p, c_i32p, c_f64p, C.POINTER(dd_diploid_pair_result), C.c_int]
    lib.dd_compute_likelihoods_realign_diploid.argtypes = [C.POINTER(dd_params), C.POINTER(dd_batch), C.POINTER(dd_result), c_f64p, c_i32p, c_i32p, c_u8p,
                                                           C.POINTER(dd_diploid_pair_result), C.POINTER(dd_realign_result), C.c_int, C.c_int, C.c_uint32]
    lib.dd_indel_keys_device.argtypes = [C.POINTER(dd_device_batch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.dd_indel_keys_host.argtypes = [C.POINTER(dd_batch), c_i16p, c_i32p, c_i16p, C.c_int]
    lib.dd_compute_likelihoods_faster_keys.argtypes = [C.POINTER(dd_params), C.POINTER(dd_batch), C.POINTER(dd_result), c_i16p, C.c_int, C.c_uint32]
    lib.dd_audit_select.argtypes = [C.POINTER(dd_params), C.POINTER(dd_batch), c_u8p, C.c_uint64, C.c_int32, c_u8p, c_i64p, c_i64p, c_i64p,
                                    C.POINTER(dd_audit_sizes)]
    lib.dd_audit_workspace_bytes.argtypes = [C.POINTER(dd_params), C.POINTER(dd_audit_view)]
    lib.dd_audit_workspace_bytes.restype = C.c_size_t
    lib.dd_audit_device.argtypes = [C.POINTER(dd_params), C.POINTER(dd_device_batch), C.POINTER(dd_device_result), C.POINTER(dd_audit_view),
                                    C.POINTER(dd_device_result), C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.dd_audit_last_launch.argtypes = [C.POINTER(C.c_int64 * len(AUDIT_LOG_FIELDS))]
    lib.dd_audit_last_launch.restype = None
    lib.dd_audit_compare_host.argtypes = [C.POINTER(dd_batch), C.POINTER(dd_result), C.POINTER(dd_audit_view), C.POINTER(dd_result), C.c_void_p,
                                          C.c_int64]
    lib.dd_compute_likelihoods_audit.argtypes = [C.POINTER(dd_params), C.POINTER(dd_batch), C.POINTER(dd_result), C.c_int, C.c_uint32, C.c_uint64,
                                                 C.c_int32, C.c_void_p, C.c_int64]
    lib.dd_audit_inject_next.argtypes = [C.c_int]
    lib.dd_audit_inject_next.restype = None
    lib.dd_audit_select_faster.argtypes = [C.POINTER(dd_params), C.POINTER(dd_batch), c_u8p, C.c_uint32, C.c_uint64, C.c_int32, c_u8p, c_i64p, c_i64p,
                                           c_i64p, C.POINTER(dd_audit_sizes)]
    lib.dd_audit_workspace_bytes_faster.argtypes = lib.dd_audit_workspace_bytes.argtypes
    lib.dd_audit_workspace_bytes_faster.restype = C.c_size_t
    lib.dd_audit_device_faster.argtypes = lib.dd_audit_device.argtypes
    lib.dd_audit_last_launch_faster.argtypes = lib.dd_audit_last_launch.argtypes
    lib.dd_audit_last_launch_faster.restype = None
    lib.dd_audit_shadow_faster_host.argtypes = [C.POINTER(dd_params), C.POINTER(dd_batch), C.POINTER(dd_audit_view), C.POINTER(dd_result)]
    lib.dd_audit_compare_host_faster.argtypes = lib.dd_audit_compare_host.argtypes
    lib.dd_compute_likelihoods_faster_audit.argtypes = [C.POINTER(dd_params), C.POINTER(dd_batch), C.POINTER(dd_result), c_i16p, C.c_int, C.c_uint32,
                                                        C.c_uint64, C.c_int32, C.c_void_p, C.c_int64]
    lib.dd_last_launch.argtypes = [C.POINTER(C.c_int32 * 8)]
    lib.dd_last_launch.restype = None
    lib.dd_launch_log.argtypes = [c_i32p, C.c_int]
    lib.dd_last_direct_outputs.argtypes = []
    lib.dd_last_direct_outputs.restype = C.c_int
    lib.dd_kernel_name.restype = C.c_char_p
    lib.dd_last_error.restype = C.c_char_p
    lib.dd_abi_version.restype = C.c_int
    lib.dd_device_count.restype = C.c_int
    _lib = lib
    return lib


def last_launch():
    """Geometry of the last launch: dict(K, D, waves, lds_block, grid, split, lds_wave, lds_shared)."""
    out = (C.c_int32 * 8)()
    load().dd_last_launch(C.byref(out))
    return dict(zip(["K", "D", "waves", "lds_block", "grid", "split", "lds_wave", "lds_shared"], list(out)))


LAUNCH_LOG_FIELDS = ["K", "pairs_per_wave", "D", "gbt", "fold", "waves", "lds_block", "grid", "split", "n_haps", "max_hap", "min_read", "max_read",
                     "waves_per_cu", "occ", "us", "dynamic", "reads_per_wave"]


def launch_log():
    """Every main-model launch of the last dd_launch_device / dd_compute_likelihoods call of this thread (dd_launch_log)."""
    import numpy as np
    buf = np.zeros((64, len(LAUNCH_LOG_FIELDS)), np.int32)
    n = load().dd_launch_log(buf.ctypes.data_as(c_i32p), 64)
    return [dict(zip(LAUNCH_LOG_FIELDS, [int(v) for v in buf[i]])) for i in range(min(n, 64))]


LONG_LOG_FIELDS = ["grid", "pairs", "max_pairs_per_wg", "ws_bytes", "K", "max_hap", "max_read", "lds_block"]
FASTER_LONG_LOG_FIELDS = ["grid", "pairs", "max_pairs_per_wg", "ws_bytes", "max_items_per_wg", "max_hap", "max_read", "lds_block"]


def _launch_log(fn, fields):
    """The records of one of the library's int64 launch logs as dicts."""
    import numpy as np
    buf = np.zeros((64, len(fields)), np.int64)
    n = fn(buf.ctypes.data_as(c_i64p), 64)
    return [dict(zip(fields, [int(v) for v in buf[i]])) for i in range(min(n, 64))]


def last_launch_of(symbol, fields):
    """This thread's last launch of one of the drawing kernels: the int64 record `symbol` (a dd_*_last_launch) fills, as a dict."""
    out = (C.c_int64 * len(fields))()
    getattr(load(), symbol)(C.byref(out))
    return dict(zip(fields, list(out)))


def stream_of(stream, device):
    """`stream`, or the current torch stream of `device` when it is None."""
    import torch
    return stream if stream is not None else torch.cuda.current_stream(device)


def long_launch_log():
    """Every long-window launch of the last dd_launch_device_long / dd_launch_device_wide / dd_compute_likelihoods_ex call of this thread
    (dd_long_launch_log).  `wide` says whether the wide build ran; K is the states per thread / 256 either way."""
    recs = _launch_log(load().dd_long_launch_log, LONG_LOG_FIELDS)
    for r in recs:
        r["wide"] = bool(r["K"] & DD_LONG_LOG_WIDE)
        r["K"] &= DD_LONG_LOG_WIDE - 1
    return recs


def faster_long_launch_log():
    """Every long-window launch of the --faster model in the last dd_launch_device_faster_long / dd_compute_likelihoods_faster_ex call of
    this thread (dd_faster_long_launch_log)."""
    return _launch_log(load().dd_faster_long_launch_log, FASTER_LONG_LOG_FIELDS)


def screen_windows_ex(params, pb, options=DD_OPT_LONG_WINDOWS):
    """dd_screen_windows_ex: (class per window, [main max hap, main max read, long max hap, long max read], unsupported count)."""
    import numpy as np
    cls = np.zeros(max(pb.n_windows, 1), np.uint8)
    mx = (C.c_int32 * 4)()
    b = pb.ctypes_batch()
    n = load().dd_screen_windows_ex(C.byref(params) if params is not None else None, C.byref(b), options, cls.ctypes.data_as(c_u8p),
                                    C.byref(mx))
    if n < 0:
        raise RuntimeError("dd_screen_windows_ex rc=%d: %s" % (n, last_error()))
    return cls[:pb.n_windows], list(mx), n


def last_error():
    return load().dd_last_error().decode()


def hpos_reference_codes(hpos):
    """hpos as the library writes it (inserted bases carry their key: DD_HPOS_INS_KEY0 - pos) -> the reference's
    MLAlignment::hpos codes (every inserted base -1)."""
    import numpy as np
    h = np.asarray(hpos).copy()
    h[h < DD_HPOS_INS_KEY0] = DD_HPOS_INS
    return h


def realign_arrays(n_reads, ops_cap):
    """Host arrays for dd_compute_likelihoods_realign: (dict(hap, status, n_ops, ops [n_reads, ops_cap], ref_off), the dd_realign_result
    that points at them).  Keep the dict alive as long as the struct is in use."""
    import numpy as np
    n = max(int(n_reads), 1)
    a = {k: np.zeros(n, np.int32) for k in ("hap", "status", "n_ops", "ref_off")}
    a["ops"] = np.zeros((n, int(ops_cap)), np.uint32)
    res = dd_realign_result(*[a[k].ctypes.data for k in REALIGN_RESULT_FIELDS])
    return {k: v[:int(n_reads)] for k, v in a.items()}, res


def diploid_pair_arrays(n_windows):
    """Host arrays for the certified MAP pair of every window: (dict(pair [n_windows, 2], state, best, gap, margin), the
    dd_diploid_pair_result that points at them).  Keep the dict alive as long as the struct is in use."""
    import numpy as np
    n = max(int(n_windows), 1)
    a = {k: np.zeros((n, 2) if k == "pair" else n, DIPLOID_PAIR_DTYPES[k]) for k in DIPLOID_PAIR_FIELDS}
    res = dd_diploid_pair_result(*[a[k].ctypes.data for k in DIPLOID_PAIR_FIELDS])
    return {k: v[:int(n_windows)] for k, v in a.items()}, res


def diploid_pairs_host(win_hap_off, win_read_off, ll, prior, status=None, nthreads=1):
    """dd_diploid_pairs_host on plain arrays: the window offsets (int32 [n_windows + 1]), ll (and status) per pair in pair order, prior laid
    out by dd_pair_sum_offsets (H * H doubles per window).  Returns dict(pair, state, best, gap, margin)."""
    import numpy as np
    ho = np.ascontiguousarray(win_hap_off, np.int32)
    ro = np.ascontiguousarray(win_read_off, np.int32)
    ll = np.ascontiguousarray(ll, np.float64)
    prior = np.ascontiguousarray(prior, np.float64)
    st = None if status is None else np.ascontiguousarray(status, np.int32)
    b = dd_batch()
    b.n_windows = len(ho) - 1
    b.win_hap_off = ho.ctypes.data_as(c_i32p)
    b.win_read_off = ro.ctypes.data_as(c_i32p)
    out, res = diploid_pair_arrays(b.n_windows)
    rc = load().dd_diploid_pairs_host(C.byref(b), ll.ctypes.data_as(c_f64p) if ll.size else None, st.ctypes.data_as(c_i32p) if st is not None else None,
                                      prior.ctypes.data_as(c_f64p) if prior.size else None, C.byref(res), int(nthreads))
    if rc != 0:
        raise RuntimeError("dd_diploid_pairs_host rc=%d: %s" % (rc, last_error()))
    return out


def indel_keys_host(pb, hpos, status=None, nthreads=1):
    """dd_indel_keys_host on a PackedBatch: the --faster model's indel-map key count of every pair (int16 [n_pairs]) from hpos (int16, laid
    out like dd_result.hpos) and, when given, the pairs' status (int32 [n_pairs])."""
    import numpy as np
    hp = np.ascontiguousarray(hpos, np.int16)
    st = None if status is None else np.ascontiguousarray(status, np.int32)
    if hp.size < pb.hpos_len or (st is not None and st.size < pb.n_pairs):
        raise ValueError("hpos / status shorter than the batch's")
    out = np.zeros(max(pb.n_pairs, 1), np.int16)
    b = pb.ctypes_batch()
    rc = load().dd_indel_keys_host(C.byref(b), hp.ctypes.data_as(c_i16p) if hp.size else None, st.ctypes.data_as(c_i32p) if st is not None else None,
                                   out.ctypes.data_as(c_i16p), int(nthreads))
    if rc != 0:
        raise RuntimeError("dd_indel_keys_host rc=%d: %s" % (rc, last_error()))
    return out[:pb.n_pairs]


class AuditSample:
    """dd_audit_select on a PackedBatch: audit_class (uint8 [n_windows]), pair_off / hpos_off / varcov_off (int64 [n_windows + 1]), sizes
    (dd_audit_sizes), n_eligible, and `chosen`, the chosen windows' indices.  view() points a dd_audit_view at the host arrays (keep the
    sample alive while it is in use).  faster=True: dd_audit_select_faster, the sample of a --faster launch, with `options` (0 or
    DD_OPT_LONG_WINDOWS_FASTER: long windows are eligible too)."""

    def __init__(self, params, pb, n_want, seed=0, win_class=None, faster=False, options=0):
        import numpy as np
        W = pb.n_windows
        self.n_windows, self.n_qual = W, int(pb.ctypes_batch().n_qual)
        self.audit_class = np.zeros(max(W, 1), np.uint8)
        self.pair_off, self.hpos_off, self.varcov_off = (np.zeros(W + 1, np.int64) for _ in range(3))
        self.sizes = dd_audit_sizes()
        wc = None if win_class is None else np.ascontiguousarray(win_class, np.uint8)
        b = pb.ctypes_batch()
        head = [C.byref(params), C.byref(b), wc.ctypes.data_as(c_u8p) if wc is not None else None]
        tail = [int(seed) & (2 ** 64 - 1), int(n_want), self.audit_class.ctypes.data_as(c_u8p), self.pair_off.ctypes.data_as(c_i64p),
                self.hpos_off.ctypes.data_as(c_i64p), self.varcov_off.ctypes.data_as(c_i64p), C.byref(self.sizes)]
        self.faster = bool(faster)
        if self.faster:
            rc = load().dd_audit_select_faster(*head, int(options), *tail)
        else:
            rc = load().dd_audit_select(*head, *tail)
        if rc < 0:
            raise RuntimeError("dd_audit_select%s rc=%d: %s" % ("_faster" if self.faster else "", rc, last_error()))
        self.n_eligible = rc
        self.audit_class = self.audit_class[:W]
        self.chosen = np.nonzero(self.audit_class == DD_WIN_LONG)[0]

    def view(self, addresses=None):
        """A dd_audit_view of the host arrays, or of `addresses` = (audit_class, pair_off, hpos_off, varcov_off) raw device addresses."""
        if addresses is None:
            addresses = [a.ctypes.data for a in (self.audit_class, self.pair_off, self.hpos_off, self.varcov_off)]
        return dd_audit_view(self.n_windows, self.n_qual, *addresses, self.sizes)


def audit_report_buffer(max_records):
    """Host memory for a report with room for max_records records (uint8 array, 8-byte aligned)."""
    import numpy as np
    return np.zeros((C.sizeof(dd_audit_report) + int(max_records) * C.sizeof(dd_audit_record) + 7) // 8, np.int64).view(np.uint8)


def audit_report(buf, max_records):
    """A report's bytes (numpy uint8) as dict(n_pairs, n_diff, diff {field: count}, compared {field: count}, records [dict(window, field
    name, pair, index, primary_bits, shadow_bits)]): the first min(n_diff, max_records) records."""
    import numpy as np
    raw = np.ascontiguousarray(buf).view(np.uint8)
    hdr = dd_audit_report.from_buffer_copy(raw[:C.sizeof(dd_audit_report)].tobytes())
    n = min(int(hdr.n_diff), int(max_records))
    recs = []
    for i in range(n):
        at = C.sizeof(dd_audit_report) + i * C.sizeof(dd_audit_record)
        r = dd_audit_record.from_buffer_copy(raw[at:at + C.sizeof(dd_audit_record)].tobytes())
        recs.append(dict(window=int(r.window), field=AUDIT_FIELDS[r.field] if 0 <= r.field < DD_AUDIT_N_FIELDS else int(r.field), pair=int(r.pair),
                         index=int(r.index), primary_bits=int(r.primary_bits), shadow_bits=int(r.shadow_bits)))
    return dict(n_pairs=int(hdr.n_pairs), n_diff=int(hdr.n_diff), diff={k: int(hdr.diff[i]) for i, k in enumerate(AUDIT_FIELDS)},
                compared={k: int(hdr.compared[i]) for i, k in enumerate(AUDIT_FIELDS)}, records=recs)


def audit_compare_host(pb, primary, sample, shadow, max_records=64):
    """dd_audit_compare_host: `primary` and `shadow` are dd_result structs over host arrays (batch.alloc_result's second value, or one built
    by hand with NULL fields); returns audit_report's dict."""
    buf = audit_report_buffer(max_records)
    b = pb.ctypes_batch()
    v = sample.view()
    rc = load().dd_audit_compare_host(C.byref(b), C.byref(primary), C.byref(v), C.byref(shadow), buf.ctypes.data, int(max_records))
    if rc != 0:
        raise RuntimeError("dd_audit_compare_host rc=%d: %s" % (rc, last_error()))
    return audit_report(buf, max_records)


def audit_shadow_faster_host(params, pb, sample, shadow):
    """dd_audit_shadow_faster_host: the --faster model's shadow of `sample` (an AuditSample made with faster=True) on the CPU, written into
    `shadow`, a dd_result struct over host arrays of the sample's lengths (NULL fields are not written)."""
    b = pb.ctypes_batch()
    v = sample.view()
    rc = load().dd_audit_shadow_faster_host(C.byref(params), C.byref(b), C.byref(v), C.byref(shadow))
    if rc != 0:
        raise RuntimeError("dd_audit_shadow_faster_host rc=%d: %s" % (rc, last_error()))


def audit_compare_host_faster(pb, primary, sample, shadow, max_records=64):
    """dd_audit_compare_host_faster: audit_compare_host under the --faster model's rule."""
    buf = audit_report_buffer(max_records)
    b = pb.ctypes_batch()
    v = sample.view()
    rc = load().dd_audit_compare_host_faster(C.byref(b), C.byref(primary), C.byref(v), C.byref(shadow), buf.ctypes.data, int(max_records))
    if rc != 0:
        raise RuntimeError("dd_audit_compare_host_faster rc=%d: %s" % (rc, last_error()))
    return audit_report(buf, max_records)


def audit_last_launch_faster():
    """The shadow launch of this thread's last dd_audit_device_faster call (dd_audit_last_launch_faster)."""
    return last_launch_of("dd_audit_last_launch_faster", AUDIT_FASTER_LOG_FIELDS)


def audit_last_launch():
    """The audit's long launch of this thread's last dd_audit_device / dd_compute_likelihoods_audit call (dd_audit_last_launch)."""
    return last_launch_of("dd_audit_last_launch", AUDIT_LOG_FIELDS)


def cigar_ops(ops, n_ops):
    """One pair's operations as [(op, len)] (op 0 = M, 1 = I, 2 = D, 4 = S): the first n_ops words of its ops row."""
    return [(int(v) & 15, int(v) >> 4) for v in list(ops)[:int(n_ops)]]


def cigar_string(ops, n_ops):
    """One pair's CIGAR as text, e.g. '3S40M2I57M'; needs n_ops <= len(ops) (DD_CIGAR_OVERFLOW pairs hold only their first ops_cap operations)."""
    if int(n_ops) > len(ops):
        raise ValueError("the pair has %d operations, %d were kept (DD_CIGAR_OVERFLOW)" % (int(n_ops), len(ops)))
    return "".join("%d%s" % (ln, "MIDNSHP=X"[op]) for op, ln in cigar_ops(ops, n_ops))


def kernel_source_id(kernel="dd_hmm_kernel"):
    """Identity of the sources a kernel is built from (12 hex digits of a SHA-1 over the files): profiles/*_pmc.json records it, and
    bench.py quotes a file's HBM-traffic counters only for the kernel they were measured on."""
    import hashlib
    import re
    faster = ["faster_model.h", "faster_sstate.inc", "faster_pair_end.inc", "faster_kernel.hip"]
    files = ["hmm_kernel.h"] + (faster if "faster" in kernel else ["hmm_kernel.hip"])
    h = hashlib.sha1()
    for f in files:                                # the code, not its comments or layout
        text = open(os.path.join(_HERE, "csrc", f), "r", errors="replace").read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        h.update(re.sub(r"\s+", " ", text).encode())
    return h.hexdigest()[:12]
