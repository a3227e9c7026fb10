/*
 * dindel_hmm.h — C ABI of the MI355X-native read x candidate-haplotype HMM likelihood path.
 *
 * This is the drop-in boundary for ONE hot path of genome/dindel-tgi:
 *
 *     void DetInDel::computeLikelihoods(const vector<Haplotype>& haps, const vector<Read>& reads,
 *                                       vector<vector<MLAlignment> >& liks,
 *                                       uint32_t leftPos, uint32_t rightPos, vector<int>& onHap);
 *                                                  (reference: DInDel.hpp:136, DInDel.cpp:1707-1739)
 *
 * which, per (haplotype, read) pair, constructs an ObservationModelFBMaxErr and calls
 * calcLikelihood() (reference: ObservationModelFB.cpp:1631-1829, 1057-1165, 1351-1475).
 * Everything is plain pointers and sizes; no STL, no torch types.  One call processes a BATCH of
 * windows (the reference processes one window per call; a GPU needs many to fill 256 CUs).
 *
 * Two ways in:
 *   (1) dd_compute_likelihoods()  — host pointers in, host pointers out.  The library owns device
 *       memory, H2D/D2H and the launch.  This is what the reference's C++ host would bind.
 *   (2) dd_workspace_bytes() / dd_build_tables() / dd_launch_device() — every buffer is a DEVICE
 *       pointer owned by the caller (e.g. torch tensors), launch on a caller-supplied hipStream_t.
 *       bench.py and the multi-GPU driver use this so inputs are resident in HBM when timing starts.
 *
 * There is NO CPU fallback behind this ABI: without a HIP device every compute entry point returns
 * DD_ERR_NO_DEVICE.  The CPU restatement lives in oracle/ and is test infrastructure only.
 */
#ifndef DINDEL_HMM_H
#define DINDEL_HMM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DD_ABI_VERSION 13

/* hpos[] sentinel values — reference: MLAlignment.hpp:31-34 */
#define DD_HPOS_INS (-1)
#define DD_HPOS_DEL (-2)
#define DD_HPOS_LO  (-3)
#define DD_HPOS_RO  (-4)
/* hpos[] AS WRITTEN BY THIS LIBRARY carries, for an inserted read base, the haplotype position the reference keys the
 * insertion at (`pos`, ObservationModelFB.cpp:1380 / Faster.cpp:608 — the x of the inserted state numS+x) instead of the
 * bare MLAlignment::INS: the value is DD_HPOS_INS_KEY0 - pos (pos >= 1, so <= -17).  MLAlignment::hpos only says "-1", and
 * the key cannot always be recovered from the neighbouring entries (a read that is inserted as a whole; in the --faster model
 * an insertion after bases parked on the last haplotype base), yet ml.indels is keyed by it.  A consumer that wants the
 * reference's array maps DD_HPOS_IS_INS(v) to DD_HPOS_INS (the C++ adapter does). */
#define DD_HPOS_INS_KEY0    (-16)
#define DD_HPOS_IS_INS(v)   ((v) == DD_HPOS_INS || (v) < DD_HPOS_INS_KEY0)
#define DD_HPOS_INS_POS(v)  (DD_HPOS_INS_KEY0 - (v))

/* return codes of the entry points */
#define DD_SUCCESS            0
#define DD_ERR_NO_DEVICE     -1   /* no HIP device / HIP runtime error; message via dd_last_error() */
#define DD_ERR_INVALID       -2   /* malformed batch (offsets not monotone, null pointer, ...)       */
#define DD_ERR_UNSUPPORTED   -3   /* shape or option outside what the kernels cover (see limits)     */
#define DD_ERR_HIP           -4

/* per-pair status, mapped by the host adapter to the reference's throw strings / exit:
 *   1 -> throw string("hapSize error.")   ObservationModelFB.cpp:47
 *   2 -> throw string("Nan detected")     DInDel.cpp:1732-1735
 *   3 -> "Likelihood>0", exit(1)          DInDel.cpp:1722-1731                                   */
#define DD_PAIR_OK            0
#define DD_PAIR_HAPSIZE       1
#define DD_PAIR_NAN           2
#define DD_PAIR_LLPOS         3
#define DD_PAIR_UNSUPPORTED   4   /* the pair's WINDOW has a shape outside the kernel limits below (or an empty read / haplotype): none of
                                     its pairs is computed (ll = 0, offHap = offHapHMQ = 1, onHap = 0, the other outputs unwritten); every
                                     other window of the batch is processed normally.  The reference has no such limit: the C++ adapter
                                     reports the window like one whose likelihood step threw (skipped row, DInDel.cpp:1369-1374). */

/* kernel limits (screened per window on the host before launch: dd_screen_windows) */
#define DD_MAX_HAP_LEN      766   /* numS = Hs+2 <= 64 lanes x 12 positions                         */
#define DD_MAX_READ_LEN    1024
#define DD_MAX_LENGTH_DEL    31   /* D = maxLengthDel + 1 <= 32.  0..11 run the specialised D = 6 / 11 / 12 builds; 12..31 one D = 32 build (correct, not tuned;
                                     haplotypes up to 574 bp there).  Above 31: opt-in, DD_OPT_WIDE_DELETIONS (the long-window kernel's wide build) */
#define DD_WIDE_MAX_LENGTH_DEL 2147483645   /* INT32_MAX - 2: D = maxLengthDel + 1 and numT = maxLengthDel + 2 stay 32-bit counts */
/* limits of the long-window path (opt-in: DD_OPT_LONG_WINDOWS); numS = Hs+2 <= 4,096 states */
#define DD_LONG_MAX_HAP_LEN  4094
#define DD_LONG_MAX_READ_LEN 4096
#define DD_MAX_QUAL_TABLE   256
#define DD_HP_TABLE          64   /* homopolymer run lengths >= 52 are all capped at 0.99            */

/* Mirrors the fields of ObservationModelParameters the path reads — ObservationModel.hpp:28-99.
 * Every entry point that takes a dd_params refuses, with DD_ERR_INVALID and a dd_last_error() that names the field, a value that would put
 * a NaN into the tables of dd_build_tables: pError outside (0,1); pMut or pFirstgLO outside [0,1]; mapQualThreshold or capMapQualFast
 * negative; a NaN in any of these or in checkBaseQualThreshold.  (maxLengthDel outside [0,31] and forceReadOnHaplotype: DD_ERR_UNSUPPORTED.
 * An entry that takes option bits lets maxLengthDel 32..DD_WIDE_MAX_LENGTH_DEL pass when DD_OPT_WIDE_DELETIONS is among them — see "wide
 * deletions" below; a larger value is then DD_ERR_INVALID.  The reference takes any value: its only check is maxLengthDel > hapSize,
 * DD_PAIR_HAPSIZE for that pair.) */
typedef struct dd_params {
    double  pError;                  /* probability of a read indel                                  */
    double  pMut;                    /* probability of a mutation in the read                        */
    double  pFirstgLO;               /* P(first on-haplotype base | left of haplotype) = 0.01        */
    double  mapQualThreshold;        /* phred cap on the read mapping quality ("capMapQualThreshold") */
    double  checkBaseQualThreshold;  /* 0.95: base-quality threshold for nBQT / nmmBQT / mLogBQ      */
    int32_t maxLengthDel;            /* = maxLengthIndel; numT = maxLengthDel+2                      */
    int32_t padCover;                /* "flankRefSeq"                                                */
    int32_t bMid;                    /* -1 = compute from overlap (ObservationModelFB.cpp:96)        */
    int32_t forceReadOnHaplotype;    /* ObservationModelFB.cpp:307-316                               */
    int32_t mapUnmappedReads;        /* 1: add the library insert-size prior of paired reads at the join (ObservationModelFB.cpp:279-292;
                                        the CLI sets it with --libFile, DInDel.cpp:4268-4272); needs the mate / library arrays of dd_batch */
    int32_t maxMismatch;             /* "flankMaxMismatch": used only by the filterHaplotypes coverage flags */
    double  capMapQualFast;          /* phred cap on the mapping quality in the --faster model (Faster.cpp:117); 40 / CLI 45 */
} dd_params;

/* ObservationModelParameters::setDefaultValues() — ObservationModel.hpp:39-64 */
void dd_params_struct_defaults(dd_params *p);
/* the set main() installs from the CLI defaults — DInDel.cpp:3937-3949, 4122-4157 */
void dd_params_cli_defaults(dd_params *p);

/*
 * One batch = n_windows windows, CSR-packed.  Window w owns haplotypes [win_hap_off[w], win_hap_off[w+1])
 * and reads [win_read_off[w], win_read_off[w+1]).  Pairs are produced hap-major then read, like
 * liks[hidx][r]:   pair(w,h,r) = win_pair_off[w] + h * R_w + r .
 *
 * Base qualities and mapping qualities are passed as one-byte indices into small tables of the
 * probabilities the reference stores in Read::qual / Read::mapQual (Read.hpp:127-148): BAM gives
 * integer phred, so at most 94 / 256 distinct values occur; the host adapter dedups arbitrary
 * doubles.  The logs of those probabilities are taken ON THE HOST with libm (dd_build_tables) so
 * that the device does only add / compare / select and cannot differ from glibc's log().
 */
typedef struct dd_batch {
    int32_t        n_windows;
    const int32_t *win_hap_off;    /* [n_windows+1]                                                 */
    const int32_t *win_read_off;   /* [n_windows+1]                                                 */
    const uint32_t*win_hap_start;  /* [n_windows]   leftPos = hapStart of every model in the window  */

    const int32_t *hap_seq_off;    /* [n_haps+1]    into hap_seq                                    */
    const char    *hap_seq;        /* haplotype bases, any byte; 'N' matches everything              */
    const int32_t *hap_var_off;    /* [n_haps+1]    into hap_var (units: variants); may be NULL      */
    const int32_t *hap_var;        /* per variant of the HAPLOTYPE: {startRead, endRead}
                                      (AlignedVariant, Variant.hpp:125-128): hap.indels in map order
                                      then hap.snps in map order — ObservationModelFB.cpp:1465-1472  */

    const int32_t *read_seq_off;   /* [n_reads+1]   into read_seq / read_qidx                       */
    const char    *read_seq;       /* read bases                                                     */
    const uint8_t *read_qidx;      /* per base: index into qual_table                                */
    const uint8_t *read_mqidx;     /* [n_reads]     index into mapq_table                            */
    const uint32_t*read_start;     /* [n_reads]     uint32_t(read.posStat.first)                     */
    const uint8_t *read_flags;     /* [n_reads]     DD_READ_* bits; bit0 = read.isUnmapped() (BAM flag 0x4) */

    int32_t        n_qual;  const double *qual_table;  /* P(base correct), Read.hpp:143-148          */
    int32_t        n_mapq;  const double *mapq_table;  /* read.mapQual,    Read.hpp:127-131          */

    const int32_t *hap_var_flank;  /* optional (NULL = none), per variant of hap_var, 3 ints:
                                      {getLeftFlankRead(), getRightFlankRead(), kind}, kind 1 = DEL, 2 = INS,
                                      0 = neither (SNP entries): inputs of filterHaplotypes, DInDel.cpp:1973-1976 */

    /* Only read when dd_params.mapUnmappedReads != 0 (NULL otherwise): what computeBMidPrior takes from the mate and the
     * read's library (ObservationModelFB.cpp:279-292, Read.hpp:162-204,426, Library.hpp:60-66). */
    const int32_t *read_mate_pos;  /* [n_reads]     read.matePos                                     */
    const int32_t *read_mate_len;  /* [n_reads]     read.mateLen, -1 = unknown (no prior for that read) */
    const uint8_t *read_lib;       /* [n_reads]     index of read.getLibrary() in the tables below   */
    int32_t        n_libs;
    const int32_t *lib_off;        /* [n_libs+1]    into lib_prob; a library has maxins = lib_off[i+1]-lib_off[i] >= 1 entries */
    const double  *lib_prob;       /* Library::getProb(x) for x = 0..maxins-1 (normalised, floored at 1e-10) */
    const double  *lib_p95;        /* [n_libs]      Library::getNinetyFifthPctProb()                 */
} dd_batch;

/* read_flags bits (BAM flag bits the path looks at: Read.hpp:201-204, ObservationModelFB.cpp:56,279-281) */
#define DD_READ_UNMAPPED       1   /* read.isUnmapped()                                    */
#define DD_READ_PAIRED         2   /* read.isPaired()                                      */
#define DD_READ_MATE_UNMAPPED  4   /* read.mateIsUnmapped()                                */
#define DD_READ_MATE_REVERSE   8   /* read.mateIsReverse()                                 */
#define DD_READ_MATE_SAME_TID 16   /* bam->core.tid == bam->core.mtid                      */

/* Per (window,hap,read) pair, in pair order.  Any output pointer may be NULL (then not written),
 * except ll and status. Mirrors MLAlignment (MLAlignment.hpp:28-76).  onHap is derived from offHapHMQ on the device: the
 * device-pointer entries (dd_launch_device*) write it only when both pointers are given; the host-pointer entries keep a
 * device copy of offHapHMQ of their own when the caller passes NULL for it. */
typedef struct dd_result {
    double  *ll, *llOn, *llOff, *mLogBQ;
    uint8_t *offHap, *offHapHMQ;
    int16_t *numIndels, *numMismatch, *nBQT, *nmmBQT, *nMMLeft, *nMMRight, *firstBase, *lastBase;
    int16_t *hpos;        /* L entries per pair, at  hpos_off(w) + h*SL_w + (read_seq_off[r]-read_seq_off[r0(w)]),
                             SL_w = total read bases of window w;  >=0 hap index, -3 LO, -4 RO,
                             inserted base: DD_HPOS_INS_KEY0 - pos (see DD_HPOS_INS_POS) */
    uint8_t *var_covered; /* per (pair, variant of that hap): hapIndelCovered / hapSNPCovered        */
    int32_t *status;      /* DD_PAIR_*                                                               */
    uint8_t *onHap;       /* [n_reads] 1 iff any hap of the window has !offHapHMQ (DInDel.cpp:1720)  */
    uint8_t *var_fcov;    /* next row N1, same indexing as var_covered: 1 iff the read counts as covering the
                             haplotype's indel in DetInDel::filterHaplotypes (DInDel.cpp:1951-2062): read selected
                             (!offHapHMQ && numIndels==0), every haplotype base of [leftFlank-padCover,
                             rightFlank+padCover] aligned to, at most maxMismatch mismatches there.  Needs
                             dd_batch.hap_var_flank.  Two undefined behaviours of the reference loop are not reproduced:
                             it reads hpos[L], one past the end; and when leftFlank-padCover < 0 it would count the
                             negative hpos sentinels as covered positions and index the haplotype sequence with them —
                             here such an interval is simply never covered.  All pairs of a DD_PAIR_HAPSIZE haplotype get 0. */
} dd_result;

/* sizes derived from a batch (host-side, O(n_windows + n_haps)) */
typedef struct dd_sizes {
    int64_t n_haps, n_reads, n_pairs;
    int64_t hap_bases, read_bases;
    int64_t hpos_len;        /* total int16 entries of dd_result.hpos                                */
    int64_t var_cov_len;     /* total bytes of dd_result.var_covered                                 */
    int64_t cells;           /* sum over pairs of L * Hs  (the metric's "cell")                      */
    int32_t max_hap_len, max_read_len;
} dd_sizes;

int dd_batch_sizes(const dd_batch *b, dd_sizes *out);

/* Per-window shape screen: win_skip[w] = 1 iff window w holds a haplotype longer than DD_MAX_HAP_LEN, a read longer than
 * DD_MAX_READ_LEN, an empty haplotype / read, or a haplotype byte that dd_build_symbol_lut could not number (more than 26
 * distinct non-ACGTN values in the batch); its pairs get DD_PAIR_UNSUPPORTED instead of failing the whole batch.
 * max_len_out[2] (may be NULL) = longest haplotype / read among the windows that pass.  Returns the number of skipped
 * windows (>= 0) or a DD_ERR_* code.  dd_compute_likelihoods does this by itself; callers of dd_launch_device upload
 * win_skip (dd_device_batch.win_skip) and plan with the returned maxima. */
int dd_screen_windows(const dd_batch *b, uint8_t *win_skip, int32_t max_len_out[2]);

/* Offsets a consumer needs to index the ragged outputs; arrays sized [n_windows+1]. */
int dd_batch_offsets(const dd_batch *b, int64_t *win_pair_off, int64_t *win_hpos_off, int64_t *win_varcov_off);

/* ---- (1) host-pointer entry point --------------------------------------------------------- */
/* device >= 0: HIP device ordinal.  Synchronous.  Replaces the body of computeLikelihoods for a
 * batch of windows. */
int dd_compute_likelihoods(const dd_params *p, const dd_batch *b, dd_result *r, int device);
/* Several devices of ONE process (the reference is one process, DInDel.cpp:4074): the batch is cut into n_devices contiguous
 * window blocks balanced by cells (sum over a window's pairs of L * Hs) — dd_partition_windows — and block i
 * runs on devices[i] under its own host thread, device arena and streams; every block writes straight into the caller's
 * arrays at its windows' offsets, so the result is the single-device result bit for bit and no collective is needed.
 * A device may be named more than once (its blocks then run concurrently on it).  Returns the first non-zero code of a block. */
int dd_compute_likelihoods_multi(const dd_params *p, const dd_batch *b, dd_result *r, const int *devices, int n_devices);
/* bounds[n_parts+1]: block i = windows [bounds[i], bounds[i+1]) */
int dd_partition_windows(const dd_batch *b, int n_parts, int32_t *bounds);

/* The host-pointer entry points keep a device arena, a pinned staging mirror and two streams per host thread between
 * calls (one window per call would otherwise be all allocation overhead); this frees them. */
void dd_release_cache(void);
/* Makes the calling thread's cache on `device` at least this big now (device arena, pinned staging mirror) and creates its streams:
 * a caller that knows work is coming can pay the allocations while its first batch is still being prepared.  Optional. */
int dd_reserve_cache(int device, size_t device_bytes, size_t pinned_bytes);
/* Page-locked host memory for the arrays of dd_batch / dd_result: with it the H2D / D2H copies of dd_compute_likelihoods run
 * at full link speed and truly overlap the kernels (pageable memory is staged by the runtime).  Optional: any host pointer
 * works.  dd_host_alloc returns NULL when there is no device or the allocation fails.  Output arrays of dd_compute_likelihoods that
 * lie in such memory are written by the kernels directly (see dd_last_direct_outputs). */
void *dd_host_alloc(size_t bytes);
void dd_host_free(void *p);

/* ---- (2) device-pointer entry points ------------------------------------------------------ */
/* Table block built on the host with libm (emission logs per quality, bMid priors per mapping
 * quality, homopolymer indel-error logs, transition constants).  Returns number of doubles written
 * (<= DD_TABLE_DOUBLES); `out` is host memory that the caller copies to the device. */
#define DD_TABLE_DOUBLES (32 + 4*DD_MAX_QUAL_TABLE + 4*DD_MAX_QUAL_TABLE + 2*DD_HP_TABLE + 2*DD_MAX_QUAL_TABLE + 2*DD_MAX_QUAL_TABLE + 64)
int dd_build_tables(const dd_params *p, const double *qual_table, int n_qual,
                    const double *mapq_table, int n_mapq, double *out);
/* The same with option bits (0 or DD_OPT_WIDE_DELETIONS, below): the tables do not depend on maxLengthDel, the bit only lets a value
 * above 31 pass the parameter check. */
int dd_build_tables_ex(const dd_params *p, const double *qual_table, int n_qual,
                       const double *mapq_table, int n_mapq, double *out, uint32_t options);

/* Bases are compared as characters, as in the reference (hap[y]==nuc || hap[y]=='N', ObservationModelFB.cpp:246): any
 * byte may occur in reads and haplotypes (IUPAC codes, soft-masked lower case).  This builds the byte -> symbol-id table
 * the main kernel uses (A,C,G,T -> 0..3, N -> 4, other bytes present in a haplotype of the batch -> 5..30, the rest -> 31);
 * out[256].  With more than 26 distinct non-ACGTN haplotype bytes in one batch the values beyond the 26th (in byte order) get no id:
 * dd_screen_windows flags the windows that hold one (DD_PAIR_UNSUPPORTED for those windows, not an error of the call). */
int dd_build_symbol_lut(const dd_batch *b, uint8_t *out);

/* log(Library::getProb(x)) for every entry of dd_batch.lib_prob (logprob_out[lib_off[n_libs]]) and
 * log(getNinetyFifthPctProb()) per library (log95_out[n_libs]), taken with libm on the host. */
int dd_build_library_tables(const dd_batch *b, double *logprob_out, double *log95_out);

/* Host-side derived index arrays the kernels need, sized by the caller:
 * hap_window[n_haps], win_pair_off[n_windows+1], win_hpos_off[n_windows+1], win_varcov_off[n_windows+1] */
int dd_build_index(const dd_batch *b, int32_t *hap_window, int64_t *win_pair_off,
                   int64_t *win_hpos_off, int64_t *win_varcov_off);

/* Ragged batches: every launch covers one (lane tiling of the haplotypes, read class), so one long haplotype or read does not put the
 * whole batch on the slower build.  The haplotype classes are the lane tilings (<= 30, 62, 94, 126, 158, 190, 222, 254, 318, ... 766 bp).
 * Read classes of a tiling: 0 = the reads of windows whose longest read (up to 160 bp) is <= T, 1 = the reads up to 160 bp of the other
 * windows, 2 = reads longer than 160 bp; T = the longest read whose back-pointer tile still fits LDS at full occupancy for that tiling and
 * these params (no class 0 / 1 distinction when p is NULL).  A haplotype is listed in a launch only if its window has reads for it.
 * dd_compute_likelihoods does this by itself; for dd_launch_device the caller builds the summary once on the host
 * (dd_build_length_classes), uploads hap_class_list and hands both over in dd_device_batch. */
#define DD_N_HAP_CLASSES 16
#define DD_N_READ_CLASSES 3
typedef struct dd_launch_class {
    int32_t list_off, list_len;         /* hap_class_list[list_off .. list_off + list_len): the launch's haplotypes, ascending            */
    int32_t hap_class;                  /* lane tiling (index of the haplotype-length class)                                              */
    int32_t max_hap_len;                /* longest haplotype of the list                                                                  */
    int32_t min_read_len, max_read_len; /* shortest admissible read / longest read present                                                */
    int32_t max_window_reads, avg_window_reads;   /* reads of the interval per window of the list: most, mean                             */
    int32_t avg_read_len;               /* mean length of those reads                                                                      */
} dd_launch_class;
typedef struct dd_length_classes {
    int32_t n_launches;                 /* non-empty (tiling, interval) combinations                                                      */
    int32_t list_len;                   /* entries of hap_class_list in use (<= n_haps * DD_N_READ_CLASSES)                               */
    dd_launch_class launch[DD_N_HAP_CLASSES * DD_N_READ_CLASSES];
} dd_length_classes;
/* hap_class_list[n_haps * DD_N_READ_CLASSES] (host memory; copy list_len entries to the device).
 * win_skip (may be NULL = none): dd_screen_windows' flags; haplotypes of skipped windows ride in the first launch without counting
 * towards its maxima (the kernel only marks their pairs), and their reads do not count. */
int dd_build_length_classes(const dd_batch *b, const uint8_t *win_skip, const dd_params *p, int32_t *hap_class_list, dd_length_classes *out);

typedef struct dd_device_batch {   /* all DEVICE pointers; same meaning as dd_batch */
    int32_t n_windows, n_haps, n_reads;
    int32_t max_hap_len, max_read_len;
    int32_t max_window_reads;       /* most reads a window has (0 = not known: every haplotype's reads are then dealt to the same number of workgroups) */
    const int32_t *win_hap_off, *win_read_off; const uint32_t *win_hap_start;
    const int32_t *hap_seq_off; const char *hap_seq; const int32_t *hap_var_off, *hap_var;
    const int32_t *read_seq_off; const char *read_seq; const uint8_t *read_qidx, *read_mqidx;
    const uint32_t *read_start; const uint8_t *read_flags;
    const int32_t *hap_window; const int64_t *win_pair_off, *win_hpos_off, *win_varcov_off;
    const double  *tables;          /* DD_TABLE_DOUBLES doubles from dd_build_tables               */
    int32_t n_qual, n_mapq;
    const int32_t *hap_var_flank;   /* optional, see dd_batch */
    const uint8_t *sym_lut;         /* optional: 256 bytes from dd_build_symbol_lut; NULL = haplotypes hold A,C,G,T,N only */
    /* mapUnmappedReads only (NULL otherwise): device copies of dd_batch's mate arrays and the log tables of
     * dd_build_library_tables */
    const int32_t *read_mate_pos, *read_mate_len; const uint8_t *read_lib;
    const int32_t *lib_off; const double *lib_logprob, *lib_log95;
    /* optional, both or neither: per-class launches for ragged batches (main model only) */
    const int32_t *hap_class_list;          /* DEVICE copy of dd_build_length_classes' list */
    const dd_length_classes *classes;       /* HOST pointer */
    const uint8_t *win_skip;                /* optional: DEVICE copy of dd_screen_windows' flags [n_windows]; NULL = every window is
                                               within the limits (max_hap_len / max_read_len then cover the whole batch).  May be
                                               dd_screen_windows_ex's classes: the main kernels skip every non-zero value */
    int32_t long_max_hap_len, long_max_read_len;   /* long path only (dd_workspace_bytes_long / dd_launch_device_long): the maxima over
                                                      its windows, dd_screen_windows_ex's max_len_out[2..3]; 0 = none */
} dd_device_batch;

/* bytes of device scratch dd_launch_device needs for this shape: the back-pointer tiles of the HBM-scratch builds behind a 256-byte header whose
 * first word is the item counter a launch zeroes (hipMemsetAsync on `stream`) and its workgroups draw from — never 0, and never shared by two
 * launches that may run at the same time (one workspace per stream) */
size_t dd_workspace_bytes(const dd_params *p, const dd_device_batch *b);

/* Enqueue the whole path for the batch on `stream` (a hipStream_t, may be NULL = default stream).
 * Result pointers are DEVICE pointers.  Asynchronous; no allocation, no synchronisation. */
int dd_launch_device(const dd_params *p, const dd_device_batch *b, const dd_result *r,
                     void *workspace, size_t workspace_bytes, void *stream);

/* ---- long windows (opt-in) ----------------------------------------------------------------- */
/* The main kernels cover haplotypes up to DD_MAX_HAP_LEN, reads up to DD_MAX_READ_LEN, and with maxLengthDel >= 12 haplotypes up to 574 bp.
 * With DD_OPT_LONG_WINDOWS a window outside those limits but inside DD_LONG_MAX_HAP_LEN / DD_LONG_MAX_READ_LEN (any maxLengthDel 0..31; above 31 see "wide deletions" below) is
 * computed by a kernel of its own (one workgroup per pair), launched after the main launch: the same outputs, bit for bit, as the main
 * kernels would give (main model only; the --faster model has an option of its own, DD_OPT_LONG_WINDOWS_FASTER below).  Without the option
 * nothing changes. */
#define DD_OPT_LONG_WINDOWS 1u
#define DD_WIN_MAIN 0          /* dd_screen_windows_ex classes */
#define DD_WIN_UNSUPPORTED 1
#define DD_WIN_LONG 2
/* win_class[w]: DD_WIN_MAIN, DD_WIN_UNSUPPORTED (DD_PAIR_UNSUPPORTED, as dd_screen_windows flags it) or, with DD_OPT_LONG_WINDOWS,
 * DD_WIN_LONG — a haplotype > DD_MAX_HAP_LEN, a read > DD_MAX_READ_LEN, or (p->maxLengthDel >= 12) a haplotype > 574 bp, within the long
 * limits.  Empty reads / haplotypes and haplotype bytes without a symbol id stay DD_WIN_UNSUPPORTED.  max_len_out[4] (may be NULL): longest
 * haplotype / read of the DD_WIN_MAIN windows with pairs, then of the DD_WIN_LONG ones.  Returns the number of DD_WIN_UNSUPPORTED windows.
 * options = 0: win_class and max_len_out[0..1] are dd_screen_windows' (p may then be NULL). */
int dd_screen_windows_ex(const dd_params *p, const dd_batch *b, uint32_t options, uint8_t *win_class, int32_t max_len_out[4]);
/* dd_compute_likelihoods with options; options = 0 is dd_compute_likelihoods. */
int dd_compute_likelihoods_ex(const dd_params *p, const dd_batch *b, dd_result *r, int device, uint32_t options);
/* Device-pointer path: b->win_skip = DEVICE copy of dd_screen_windows_ex's classes, b->long_max_hap_len / long_max_read_len its maxima.
 * Workspace: a 256-byte header (item counter, pair count, stats), the long windows' list, then one back-pointer tile of
 * long_max_read_len x 256 K bytes (K = 1, 2, 4, 8, 16: numS <= 256 K) per workgroup of the persistent grid.  The grid is the chip's
 * resident workgroups, shrunk so that the workspace stays within DD_LONG_WS_BUDGET (at least one workgroup: the maximum shape needs 16 MiB).
 * Never shared by two launches that may run at the same time. */
#define DD_LONG_WS_BUDGET ((size_t)512 << 20)
size_t dd_workspace_bytes_long(const dd_params *p, const dd_device_batch *b);
/* Enqueue the long kernel for the DD_WIN_LONG windows on `stream`, AFTER dd_launch_device on the same batch and stream: it overwrites its
 * windows' placeholder outputs and (when r->onHap and r->offHapHMQ are given) their reads' onHap.  No-op without long windows. */
int dd_launch_device_long(const dd_params *p, const dd_device_batch *b, const dd_result *r, void *workspace, size_t workspace_bytes, void *stream);
/* Every long launch of the last dd_launch_device_long / dd_compute_likelihoods_ex call on this host thread: records of DD_LONG_LOG_FIELDS
 * int64 {grid, pairs computed, most pairs one workgroup took, workspace bytes, K (states per thread / 256), long windows' longest
 * haplotype, longest read, LDS bytes per workgroup}.  The two counters are read from device memory (the workspace header, or the
 * host path's own copy): this synchronises the launch's stream, and for dd_launch_device_long the workspace must still be allocated.
 * Returns the number of launches. */
#define DD_LONG_LOG_FIELDS 8
#define DD_LONG_LOG_WIDE 256   /* added to the K field of a record when the wide build ran (below) */
int dd_long_launch_log(int64_t *out, int max_records);

/* ---- wide deletions (opt-in): maxLengthDel above 31 ---------------------------------------- */
/* No main-kernel build holds a jump of more than 32 states.  With DD_OPT_WIDE_DELETIONS — beside DD_OPT_LONG_WINDOWS, whose kernel it uses —
 * and p->maxLengthDel in 32..DD_WIDE_MAX_LENGTH_DEL, every window within the long limits is DD_WIN_LONG (dd_screen_windows_ex) and is computed
 * by the wide build of the long-window kernel: two bytes per back-pointer (12 bits of jump length), candidate loops clipped to the haplotype.
 * The same outputs, bit for bit, as the reference's model gives (oracle: ddo_batch); a pair with maxLengthDel > hapSize is DD_PAIR_HAPSIZE.
 * With maxLengthDel <= 31 the bit changes nothing anywhere.  Without the bit every entry answers as ever (DD_ERR_UNSUPPORTED above 31).
 * The bit alone, without DD_OPT_LONG_WINDOWS, is DD_ERR_INVALID for the main model's entries.  Out of scope: the audits (dd_audit_select and
 * dd_audit_select_faster refuse maxLengthDel > 31: the shadow would be the same kernel), the _multi entries, forceReadOnHaplotype.
 *
 * Host pointers: dd_compute_likelihoods_ex (and the _cigars / _realign / _realign_diploid entries) with
 * DD_OPT_LONG_WINDOWS | DD_OPT_WIDE_DELETIONS.
 * Device pointers: tables from dd_build_tables_ex, classes from dd_screen_windows_ex with both bits, then ONE launch, dd_launch_device_wide,
 * in place of dd_launch_device + dd_launch_device_long: there is no main launch for these parameters, so it also writes the placeholder of
 * every DD_WIN_UNSUPPORTED window's pairs (DD_PAIR_UNSUPPORTED, ll = 0, off the haplotype) and onHap of every read.  With
 * maxLengthDel <= 31 it is dd_launch_device_long (and dd_workspace_bytes_wide is dd_workspace_bytes_long).  A tile of the wide build is
 * long_max_read_len x 256 K x 2 bytes (the maximum shape: 32 MiB + stash per workgroup, the grid stays >= 1 within DD_LONG_WS_BUDGET).
 * dd_long_launch_log records the launch; its K field is K + DD_LONG_LOG_WIDE when the wide build ran.
 * The consumers behind a launch (dd_cigars_device, dd_realign_device, dd_diploid_pairs_device, dd_indel_keys_device, dd_pooled_em_device)
 * read outputs only and work behind it unchanged.
 * The --faster model compares maxLengthDel with the haplotype length and does nothing else with it: dd_compute_likelihoods_faster_ex,
 * dd_compute_likelihoods_faster_keys (where the bit is needed, maxLengthDel above 31; beside a smaller value it stays an unknown bit of
 * that entry, as ever) and dd_launch_device_faster_ex accept the bit, which only lifts the parameter check (both kernels run
 * unchanged; DD_OPT_LONG_WINDOWS_FASTER composes with it on the host-pointer entries). */
#define DD_OPT_WIDE_DELETIONS 4u
size_t dd_workspace_bytes_wide(const dd_params *p, const dd_device_batch *b);
int dd_launch_device_wide(const dd_params *p, const dd_device_batch *b, const dd_result *r, void *workspace, size_t workspace_bytes, void *stream);

/* ---- row A13: the --faster model ---------------------------------------------------------- */
/* Same batch in, same result layout out, but each pair is scored by ObservationModelS(hap, read, hapStart,
 * params).align(HapHash(4, hap)) — DetInDel::computeLikelihoodsFaster, reference DInDel.cpp:1790-1833
 * (Faster.cpp:42-681, Haplotype.hpp:315-384).  That model fills ll, hpos, firstBase, lastBase and the coverage
 * flags; offHap / offHapHMQ are always 0 (Faster.cpp:491,:529); llOn, llOff, numIndels, numMismatch stay 0 as MLAlignment's
 * constructor sets them (MLAlignment.hpp:35-46), and mLogBQ, nBQT, nmmBQT, nMMLeft, nMMRight — which that constructor leaves
 * uninitialised and this model never assigns — are reported as 0.  Params used: pError, pMut, maxLengthDel (size check only), padCover,
 * capMapQualFast, maxMismatch.  status: DD_PAIR_HAPSIZE (`throw string("hapSize error.")`, Faster.cpp:47) or
 * DD_PAIR_NAN for a read shorter than the 4-mer (`throw string("HapHash string too short")`, Haplotype.hpp:341). */
int dd_compute_likelihoods_faster(const dd_params *p, const dd_batch *b, dd_result *r, int device);
int dd_compute_likelihoods_faster_multi(const dd_params *p, const dd_batch *b, dd_result *r, const int *devices, int n_devices);
int dd_launch_device_faster(const dd_params *p, const dd_device_batch *b, const dd_result *r, void *stream);
/* with options: 0 is dd_launch_device_faster; DD_OPT_WIDE_DELETIONS (above) lets maxLengthDel above 31 pass; any other bit is DD_ERR_INVALID */
int dd_launch_device_faster_ex(const dd_params *p, const dd_device_batch *b, const dd_result *r, void *stream, uint32_t options);

/* ---- long windows of the --faster model (opt-in, separate from DD_OPT_LONG_WINDOWS) ------- */
/* dd_faster_kernel covers haplotypes up to DD_MAX_HAP_LEN and reads up to DD_MAX_READ_LEN (its per-pair LDS area); the reference's model has
 * no such limit.  With DD_OPT_LONG_WINDOWS_FASTER a window with a haplotype of 767..DD_LONG_MAX_HAP_LEN bp or a read of
 * 1,025..DD_LONG_MAX_READ_LEN bp is computed by a kernel of its own (faster_long_kernel.hip: back-pointers and vote histogram in an HBM
 * workspace), launched after the --faster main launch: the same outputs, bit for bit, as dd_faster_kernel's arithmetic gives.  Without the
 * option nothing changes, and DD_OPT_LONG_WINDOWS has no effect on the --faster model.
 *
 * dd_screen_windows_ex with this bit classes the windows for the --faster model: DD_WIN_LONG as above, whatever maxLengthDel is (the
 * 574-bp cap of the D = 32 build is a main-model matter) and whatever bytes the haplotypes hold (this model compares bytes); max_len_out[2..3]
 * the long windows' maxima.  The classes are per model: both option bits together are DD_ERR_INVALID.
 * Out of scope: dd_compute_likelihoods_faster_multi (long windows stay skipped there); mapUnmappedReads (this model has no insert-size prior). */
#define DD_OPT_LONG_WINDOWS_FASTER 2u
/* dd_compute_likelihoods_faster with options: 0 is dd_compute_likelihoods_faster; DD_OPT_LONG_WINDOWS_FASTER computes the long windows
 * too; DD_OPT_WIDE_DELETIONS lets maxLengthDel above 31 pass; any other bit is DD_ERR_INVALID. */
int dd_compute_likelihoods_faster_ex(const dd_params *p, const dd_batch *b, dd_result *r, int device, uint32_t options);
/* Device-pointer path: b->win_skip = DEVICE copy of the classes dd_screen_windows_ex gave with DD_OPT_LONG_WINDOWS_FASTER,
 * b->long_max_hap_len / long_max_read_len its max_len_out[2..3] (a dd_device_batch is screened for one model at a time).
 * Workspace: a 256-byte header (item counter, counts, stats), the long windows' list and item offsets, then per workgroup of the persistent
 * grid 16 tiles (one per pair in flight) of 16 B per read base + 2 B per diagonal.  The grid is the chip's resident workgroups (LDS-limited,
 * at most 2 per CU) and no more than the batch can have items (n_haps x ceil(n_reads / 16)), shrunk so that the workspace stays within
 * DD_FASTER_LONG_WS_BUDGET — never below one workgroup (the maximum shape needs 1.3 MiB per workgroup).  0 when there is no long window
 * or a shape is beyond the limits.  Never shared by two launches that may run at the same time. */
#define DD_FASTER_LONG_WS_BUDGET ((size_t)512 << 20)
size_t dd_workspace_bytes_faster_long(const dd_params *p, const dd_device_batch *b);
/* Enqueue the kernel for the DD_WIN_LONG windows on `stream`, AFTER dd_launch_device_faster on the same batch and stream: it overwrites
 * its windows' placeholder outputs and (when r->onHap and r->offHapHMQ are given) their reads' onHap.  No-op without long windows; a
 * workspace that is too small is DD_ERR_INVALID. */
int dd_launch_device_faster_long(const dd_params *p, const dd_device_batch *b, const dd_result *r, void *workspace, size_t workspace_bytes,
                                 void *stream);
/* Every such launch of the last dd_launch_device_faster_long / dd_compute_likelihoods_faster_ex call on this host thread: records of
 * DD_FASTER_LONG_LOG_FIELDS int64 {grid, pairs handled, most pairs one workgroup took, workspace bytes, most items one workgroup took,
 * long windows' longest haplotype, longest read, LDS bytes per workgroup}.  The three counters are read from device memory (the workspace
 * header, or the host path's own copy): this synchronises the launch's stream, and for dd_launch_device_faster_long the workspace must
 * still be allocated.  Returns the number of launches. */
#define DD_FASTER_LONG_LOG_FIELDS 8
int dd_faster_long_launch_log(int64_t *out, int max_records);

/* ---- device-side getCIGAR (opt-in) --------------------------------------------------------- */
/* The CIGAR of every (haplotype, read) pair — DetInDel::getCIGAR, reference DInDel.cpp:728-882 (host/cigar.cpp restates it and is the
 * specification) — computed on the device from the hpos the likelihood kernels left there, so that a realigned BAM needs
 * 4 * ops_cap + 12 bytes per pair instead of the pair's 2 L bytes of hpos.  Nothing changes for callers that do not ask for it.
 * Per pair, in pair order (liks[h][r], like dd_result):
 *   status   DD_CIGAR_*: 0, or the string getCIGAR throws there, or DD_CIGAR_OVERFLOW, or DD_CIGAR_NOT_COMPUTED
 *   n_ops    the number of operations, also when it exceeds ops_cap (0 when status names a throw or DD_CIGAR_NOT_COMPUTED)
 *   ops      [ops_cap] per pair, BAM-encoded len << 4 | op with op 0 = M, 1 = I, 2 = D, 4 = S; the first min(n_ops, ops_cap) are written.
 *            A pair whose status names a throw has n_ops 0, but the walk may have written operations into its row before it threw: the
 *            row's contents are then unspecified.  DD_CIGAR_NOT_COMPUTED pairs' rows are never written
 *   ref_off  reference offset of the first aligned base: CIGAR::refPos = refSeqStart + ref_off; -1 when the read has no aligned base
 *            (one soft clip over the whole read; refPos stays -1 there) and whenever n_ops is 0 */
typedef struct dd_cigar_result {
    int32_t  *n_ops;
    uint32_t *ops;
    int32_t  *ref_off;
    int32_t  *status;
} dd_cigar_result;
#define DD_CIGAR_OK               0
#define DD_CIGAR_HAP_NOT_ALIGNED  1   /* "Haplotype has not been aligned!" (hap_aligned[h] == 0) */
#define DD_CIGAR_ERROR1           2   /* "Error(1)!" */
#define DD_CIGAR_ERROR2           3   /* "Error(2)!" */
#define DD_CIGAR_ERROR3           4   /* "Error(3)!" */
#define DD_CIGAR_ERROR4           5   /* "Error(4)!" */
#define DD_CIGAR_IMPOSSIBLE       6   /* "How is this possible? (1)" */
#define DD_CIGAR_OVERFLOW         7   /* n_ops > ops_cap: the first ops_cap operations are there, the caller redoes this pair on the host */
#define DD_CIGAR_NOT_COMPUTED     8   /* the pair's dd_result.status is not DD_PAIR_OK: its hpos is not read and its ops are not written */
#define DD_CIGAR_DEFAULT_OPS_CAP  8
/* Enqueue the CIGAR launch for the whole batch on `stream`, behind the likelihood launch(es) that wrote hpos_dev (dd_launch_device,
 * dd_launch_device_long, dd_launch_device_faster, dd_launch_device_faster_long alike: hpos is only read).  All DEVICE pointers:
 *   hpos_dev         dd_result.hpos as the kernels write it (inserted bases carry their key, DD_HPOS_IS_INS: read as MLAlignment::INS)
 *   status_dev       dd_result.status (NULL = every pair was computed)
 *   hap_ref_pos_dev  Haplotype::refHpos (hap.ml.hpos of the reference): one int32 per haplotype base at the haplotype's hap_seq_off —
 *                    the base's offset on the window's reference sequence (>= 0) or a negative MLAlignment code
 *   hap_aligned_dev  one byte per haplotype, 0 = "Haplotype has not been aligned!" (NULL = all aligned)
 *   out_dev          device arrays: n_ops, ref_off, status [n_pairs], ops [n_pairs * ops_cap]; ops_cap >= 1
 * Of the batch it reads n_windows, win_hap_off, win_read_off, hap_seq_off, read_seq_off, win_pair_off and win_hpos_off.  An hpos entry
 * beyond its haplotype (the host would read past the vector) is read as the haplotype's last base.  Asynchronous, no allocation. */
int dd_cigars_device(const dd_device_batch *b, const int16_t *hpos_dev, const int32_t *status_dev, const int32_t *hap_ref_pos_dev,
                     const uint8_t *hap_aligned_dev, const dd_cigar_result *out_dev, int ops_cap, void *stream);
/* Host pointers: dd_compute_likelihoods_ex (options: 0 or DD_OPT_LONG_WINDOWS) followed by the CIGAR launch; cig's arrays (host memory,
 * sized as above) are filled.  hap_ref_pos [hap_seq_off[n_haps]] is required, hap_aligned [n_haps] may be NULL (all aligned).
 * r->hpos may be NULL: the per-base alignments then stay on the device — the point of this entry.  Everything else as
 * dd_compute_likelihoods_ex. */
int dd_compute_likelihoods_cigars(const dd_params *p, const dd_batch *b, dd_result *r, const int32_t *hap_ref_pos, const uint8_t *hap_aligned,
                                  const dd_cigar_result *cig, int ops_cap, int device, uint32_t options);

/* ---- realigned reads: per-read haplotype choice and CIGAR on the device (opt-in) ------------ */
/* Which haplotype a read is realigned to, and that pair's CIGAR, chosen on the device from the ll / onHap / hpos the likelihood kernels
 * left there: 4 * ops_cap + 16 bytes per read come back instead of H * (4 * ops_cap + 12).  Both rules are compares and selects (no exp,
 * no log) and equal the host's (host/realigned_bam.cpp) bit for bit.  Read q is read r of window w with H haplotypes and R reads;
 * pair(h) = win_pair_off[w] + h * R + r, g(h) = win_hap_off[w] + h.
 *   DD_REALIGN_FIRST_MAX  the pooled rule (reference DInDel.cpp:503-511): on_hap[q] == 0 (when on_hap is given) chooses nothing
 *                         (DD_REALIGN_OFF_HAP, hap -1, n_ops 0, ref_off -1, ops row not written); otherwise the first h whose ll is
 *                         strictly greater than the running maximum, starting from -inf; h = 0 when none compares greater (all -inf; NaN
 *                         never compares greater)
 *   DD_REALIGN_PAIR       the diploid rule (DInDel.cpp:596-610): h1 = win_hap_pair[2w], h2 = win_hap_pair[2w+1]; either outside [0, H)
 *                         gives every read of the window DD_REALIGN_BAD_PAIR and hap -1.  If fabs(ll[pair(h1)] - ll[pair(h2)]) < 1e-8:
 *                         h1 when hap_n_indels[g(h1)] < hap_n_indels[g(h2)], else h2; otherwise h1 when ll[pair(h1)] > ll[pair(h2)],
 *                         else h2 (NaN and -inf - -inf fall to h2).  on_hap is not consulted
 * A window with reads and no haplotype gives DD_REALIGN_NO_HAPS.  For a chosen pair, hap is its haplotype's index inside the window and
 * status, n_ops, ops and ref_off are exactly what dd_cigars_device writes for that pair (DD_CIGAR_NOT_COMPUTED, the throw codes and
 * DD_CIGAR_OVERFLOW included), at the read's index instead of the pair's. */
typedef struct dd_realign_result {   /* per READ of the batch, in read order (win_read_off) */
    int32_t  *hap;      /* [n_reads] chosen haplotype, index inside the window; -1 where none was chosen */
    int32_t  *status;   /* [n_reads] DD_CIGAR_* of the chosen pair, or one of the DD_REALIGN_* below */
    int32_t  *n_ops;    /* [n_reads] as dd_cigar_result.n_ops */
    uint32_t *ops;      /* [n_reads * ops_cap] as dd_cigar_result.ops */
    int32_t  *ref_off;  /* [n_reads] as dd_cigar_result.ref_off */
} dd_realign_result;
#define DD_REALIGN_OFF_HAP   9    /* FIRST_MAX mode: on_hap[read] == 0: nothing chosen, nothing walked */
#define DD_REALIGN_BAD_PAIR 10    /* PAIR mode: the window's h1 or h2 is outside [0, H) */
#define DD_REALIGN_NO_HAPS  11    /* the window has reads and no haplotype */
#define DD_REALIGN_FIRST_MAX 0    /* DInDel.cpp:503-511 */
#define DD_REALIGN_PAIR      1    /* DInDel.cpp:596-610 */
/* Enqueue the realign launch for the whole batch on `stream`, behind the likelihood launch(es) that wrote ll, onHap, status and hpos (any
 * of the four, as for dd_cigars_device).  All DEVICE pointers:
 *   ll_dev            dd_result.ll
 *   on_hap_dev        dd_result.onHap, one byte per read (FIRST_MAX; NULL = every read is on a haplotype; not read in PAIR mode)
 *   win_hap_pair_dev  [2 * n_windows] the window's haplotype pair (PAIR mode, required there)
 *   hap_n_indels_dev  [n_haps] Haplotype::countIndels() per haplotype of the batch (PAIR mode, required there)
 *   hpos_dev, status_dev, hap_ref_pos_dev, hap_aligned_dev, ops_cap   as for dd_cigars_device
 *   out_dev           device arrays, every one required
 * Of the batch it reads what dd_cigars_device reads, and n_reads.  Asynchronous, no allocation. */
int dd_realign_device(const dd_device_batch *b, int mode, const double *ll_dev, const uint8_t *on_hap_dev,
                      const int32_t *win_hap_pair_dev, const int32_t *hap_n_indels_dev,
                      const int16_t *hpos_dev, const int32_t *status_dev, const int32_t *hap_ref_pos_dev,
                      const uint8_t *hap_aligned_dev, const dd_realign_result *out_dev, int ops_cap, void *stream);
/* Host pointers: dd_compute_likelihoods_ex (options: 0 or DD_OPT_LONG_WINDOWS) followed by the realign launch; out's arrays (host memory)
 * are filled.  win_hap_pair and hap_n_indels are required in PAIR mode only; FIRST_MAX consults r->onHap when the caller asks for it.
 * r->hpos may be NULL.  Everything else as dd_compute_likelihoods_cigars. */
int dd_compute_likelihoods_realign(const dd_params *p, const dd_batch *b, dd_result *r, int mode,
                                   const int32_t *win_hap_pair, const int32_t *hap_n_indels,
                                   const int32_t *hap_ref_pos, const uint8_t *hap_aligned,
                                   const dd_realign_result *out, int ops_cap, int device, uint32_t options);

/* ---- diploid realigned reads: the window's MAP haplotype pair, chosen and certified on the device (opt-in) ---------- */
/* The pair DD_REALIGN_PAIR needs is maxLikelihoodPair's argmax (host/realigned_bam.cpp, reference DInDel.cpp:3767-3831) over
 *   V[h1,h2] = sum over the window's reads, in order, of (addLogs(ll[h1,r], ll[h2,r]) + log(.5))  +  prior[h1,h2],   h1 <= h2,
 * which the host takes in glibc arithmetic.  The device takes the same sums in csrc/pooled_math.h's arithmetic (bit-equal on host and
 * device, not glibc's) with a bound eps on how far either evaluation can be from the exact value:
 *   t_r = pm_add_logs(ll[h1,r], ll[h2,r]) + pm_log(0.5);  S = sum of t_r in read order;  A = sum of |t_r|;  V = S + prior[h1,h2]
 *   eps = 2^-50 ((R + 4) A + 8 R + |prior[h1,h2]|)
 *   best   = the first pair in row-major order (h1 <= h2) with the largest V
 *   second = the first pair in row-major order, other than best, with the largest V among the others (equal values count)
 *   gap    = V_best - V_second (+inf with one pair);  margin = max(eps_best, eps_second)
 * A window is certified when gap > margin: the host's argmax is then the same pair.  Every other window is left to the host.
 * prior[win_hh_off[w] + h1 * H + h2] = getHaplotypePrior(h1, h2), the layout of dd_map_pairs_device (dd_pair_sum_offsets).
 * States, in the order they are tested:
 *   DD_DIPPAIR_NO_HAPS         the window has no haplotype
 *   DD_DIPPAIR_TOO_MANY_HAPS   more than DD_DIPPAIR_MAX_HAPS haplotypes
 *   DD_DIPPAIR_NOT_COMPUTED    some pair of the window has status != 0
 *   DD_DIPPAIR_NONFINITE       some ll of the window is NaN or +-inf, some V is NaN, or V_best is not finite (the host's
 *                              addLogs(-inf, -inf) is NaN and its sort is then unspecified)
 *   DD_DIPPAIR_TIE             gap <= margin
 *   DD_DIPPAIR_CERTIFIED       gap > margin
 * Per window: pair[2w], pair[2w+1] = best, or (-1, -1) in every state but DD_DIPPAIR_CERTIFIED (dd_realign_device then gives the
 * window's reads DD_REALIGN_BAD_PAIR and walks nothing); state[w]; best[w] = V_best, gap[w], margin[w] (0 in the four states in
 * which they were not taken).  A window without reads has V = prior. */
typedef struct dd_diploid_pair_result {
    int32_t *pair;      /* [2 * n_windows] */
    int32_t *state;     /* [n_windows] DD_DIPPAIR_* */
    double  *best;      /* [n_windows] */
    double  *gap;       /* [n_windows] */
    double  *margin;    /* [n_windows] */
} dd_diploid_pair_result;
#define DD_DIPPAIR_CERTIFIED      0
#define DD_DIPPAIR_TIE            1
#define DD_DIPPAIR_NONFINITE      2
#define DD_DIPPAIR_NOT_COMPUTED   3
#define DD_DIPPAIR_NO_HAPS        4
#define DD_DIPPAIR_TOO_MANY_HAPS  5
#define DD_DIPPAIR_MAX_HAPS     128
/* Enqueue the pair launch for the whole batch on `stream`, behind the likelihood launch(es) that wrote ll_dev and status_dev.  All DEVICE
 * pointers; status_dev may be NULL (every pair was computed), every array of out_dev is required.  Of the batch it reads n_windows,
 * win_hap_off, win_read_off and win_pair_off.  out_dev->pair can be handed to dd_realign_device (DD_REALIGN_PAIR) on the same stream.
 * Asynchronous, no allocation. */
int dd_diploid_pairs_device(const dd_device_batch *b, const int64_t *win_hh_off_dev, const double *ll_dev, const int32_t *status_dev,
                            const double *prior_dev, const dd_diploid_pair_result *out_dev, void *stream);
/* The same function on the CPU, no device needed, every output equal to the device's in every bit: host pointers, ll and status per pair in
 * pair order (status may be NULL), prior laid out by dd_pair_sum_offsets; windows spread over nthreads host threads (< 1: one). */
int dd_diploid_pairs_host(const dd_batch *b, const double *ll_host, const int32_t *status_host, const double *prior_host,
                          const dd_diploid_pair_result *out, int nthreads);
/* Host pointers: dd_compute_likelihoods_realign in DD_REALIGN_PAIR mode with the window pairs chosen on the device — on every window block's
 * stream the pair launch runs behind the block's likelihood launches and in front of its realign launch, which reads the pairs where they
 * were written; the per-window arrays of pair_out (host memory) come back with the block, the reads' rows in realign_out.  A window that is
 * not DD_DIPPAIR_CERTIFIED has the pair (-1, -1) and its reads DD_REALIGN_BAD_PAIR: the caller chooses that window's pair itself.
 * prior [sum of H_w^2] (dd_pair_sum_offsets), hap_n_indels [n_haps] and hap_ref_pos are required; r->hpos may be NULL.  A batch without
 * pairs gets its windows' states from the CPU evaluation (no device needed).  Everything else as dd_compute_likelihoods_realign. */
int dd_compute_likelihoods_realign_diploid(const dd_params *p, const dd_batch *b, dd_result *r, const double *prior, const int32_t *hap_n_indels,
                                           const int32_t *hap_ref_pos, const uint8_t *hap_aligned, const dd_diploid_pair_result *pair_out,
                                           const dd_realign_result *realign_out, int ops_cap, int device, uint32_t options);

/* ---- alignHaplotypes: candidate haplotypes against the window's reference sequence ---------- */
/* The arithmetic of DetInDel::alignHaplotypes (reference DInDel.cpp:1427-1524): SeqAn's globalAlignment with
 * Score<int>(-1, -460, -100, -960) and no free end gaps, i.e. _align_gotoh / _align_gotoh_trace of seqan/graph_align/graph_align_gotoh.h,
 * tie rules and traceback state machine included.  Row 0 (columns) is the reference window, row 1 (rows) the haplotype; both are read as
 * seqan::Dna (A/a 0, C/c 1, G/g 2, T/t/U/u 3, every other byte 0 = A).  match -1, mismatch -460, a gap of n bases -960 - 100 (n - 1).
 * A batch is n_refs reference sequences and n_pairs haplotypes, each naming its reference; all offsets are in bytes of their sequence
 * array and start at 0.  The host conversion to Haplotype::indels / snps / ml.hpos is the C++ adapter's (host/align_haplotypes.cpp). */
typedef struct dd_align_batch {
    int32_t        n_refs;
    const int32_t *ref_off;    /* [n_refs + 1] */
    const char    *ref_seq;    /* [ref_off[n_refs]] */
    int32_t        n_pairs;
    const int32_t *pair_ref;   /* [n_pairs] index of the pair's reference */
    const int32_t *hap_off;    /* [n_pairs + 1] */
    const char    *hap_seq;    /* [hap_off[n_pairs]] */
} dd_align_batch;
/* Per pair: score (the alignment's, int32) and status; per haplotype base, laid out like hap_seq: the 0-based offset of the reference
 * base it is paired with, or a negative value when it faces a gap: DD_ALIGN_GAP(n) = -1 - n, n = the number of reference bases left of
 * its column.  Reference bases no haplotype base names are deleted, and n places an inserted base among them: SeqAn writes a block
 * substitution as deletion then insertion (n = the end of the deleted run) but an overhang at the matrix edge the other way round, and
 * convertAlignment treats the two differently, so the offsets of the paired bases alone do not determine the alignment.  A pair whose
 * status is not DD_ALIGN_OK has score 0 and its ref_pos slice all -1; its neighbours are untouched. */
#define DD_ALIGN_IS_GAP(v)    ((v) < 0)
#define DD_ALIGN_GAP_REFS(v)  (-1 - (v))
typedef struct dd_align_result {
    int32_t *score;     /* [n_pairs] */
    int32_t *status;    /* [n_pairs] DD_ALIGN_* */
    int16_t *ref_pos;   /* [hap_off[n_pairs]] */
} dd_align_result;
#define DD_ALIGN_OK        0
#define DD_ALIGN_EMPTY     1   /* either sequence has length 0 (checked first) */
#define DD_ALIGN_TOO_LONG  2   /* a length above DD_LONG_MAX_HAP_LEN (device entry: above the max_*_len of the launch) */
#define DD_ALIGN_BAD_REF   3   /* device entry only: pair_ref outside [0, n_refs); the host entries return DD_ERR_INVALID instead */
/* Host pointers in, host pointers out; the library owns device memory and the launch.  DD_ERR_INVALID (before any launch) for null
 * pointers, offsets that do not start at 0 or decrease, and a pair_ref out of range; DD_ERR_NO_DEVICE without a GPU. */
int dd_align_haplotypes(const dd_align_batch *b, dd_align_result *r, int device);
/* Workspace bytes of a launch over a batch of this shape (HOST pointers; the offsets and pair_ref are read): the header and one trace tile of
 * (longest reference + 64) x (longest haplotype) bytes per wavefront of the grid, lengths above the limit not counted.  The grid is one
 * wavefront per pair, four wavefronts per workgroup, at most 2,048 workgroups, and shrinks so the tiles stay within 512 MiB, never below
 * one workgroup.  The batch's longest pair sizes every wavefront's tile and LDS rows: one 4,000-bp haplotype among 130-bp ones costs the
 * whole launch its occupancy, so a caller with such outliers gives them a launch of their own.  0 on a malformed shape (dd_last_error). */
size_t dd_align_workspace_bytes(const dd_align_batch *shape);
/* Device pointers: the arrays of b_dev and r_dev live on the device, n_refs and n_pairs are values.  max_ref_len / max_hap_len
 * (1 ... DD_LONG_MAX_HAP_LEN) size the trace tile; longer pairs come back DD_ALIGN_TOO_LONG.  The grid is what workspace_bytes allows
 * (at least the header and four tiles, else DD_ERR_INVALID; dd_align_workspace_bytes gives the full grid).  The contents of the offset
 * arrays cannot be checked here.  Asynchronous on `stream`, no allocation; the pair counter in the workspace header is zeroed on the
 * stream in front of the launch, so a workspace can be reused by consecutive launches of one stream. */
int dd_align_haplotypes_device(const dd_align_batch *b_dev, const dd_align_result *r_dev, int max_ref_len, int max_hap_len,
                               void *workspace, size_t workspace_bytes, void *stream);
/* The last alignment launch on this host thread: {grid (workgroups), wavefronts, tile bytes, LDS bytes per workgroup, pairs, workspace
 * bytes used, most pairs one wavefront drew, wavefronts stopped by the draw guard}.  The last two are read from the workspace header:
 * after dd_align_haplotypes_device this synchronises the launch's stream and the workspace must still be allocated (-1 if the read fails).
 * The guard count is 0 unless the persistent loop's draw went wrong (a wavefront that iterates more often than the batch has pairs is
 * stopped and counted): the tests assert it. */
#define DD_ALIGN_LOG_FIELDS 8
void dd_align_last_launch(int64_t out[DD_ALIGN_LOG_FIELDS]);

/* ---- indel events of an alignment: what convertAlignment puts into hap.indels, without the slice ---------- */
/* One indel of one pair, as convertAlignment (reference ObservationModelSeqAn.hpp:142-269) would record it in hap.indels: keys, types,
 * lengths and read positions only — no strings, no flanks, no SNPs.
 *   kind  DD_ALIGN_EVENT_INS or DD_ALIGN_EVENT_DEL
 *   ref   the map key: reference bases left of the event (an insertion sits in front of reference base `ref`, a deletion starts there)
 *   len   inserted haplotype bases / deleted reference bases
 *   hap   first inserted haplotype base; for a deletion the haplotype base behind it (its read positions are hap - 1 and hap)
 * Rules, walking the haplotype bases in order (upto = reference bases left of the base's column, nxt = reference bases consumed so far):
 * gap-facing bases with upto == 0 are LO and give nothing; upto > nxt in front of a base is a deletion, recorded only once a paired
 * base has been seen; a maximal run of gap-facing bases with one upto = n gives an insertion only if 0 < n < reference length (else RO);
 * reference bases behind the last haplotype base give nothing.  Events come in slice order, a deletion in front of base b before an
 * insertion that starts at b. */
typedef struct dd_align_events {
    int16_t kind, ref, len, hap;
} dd_align_events;
#define DD_ALIGN_EVENT_INS 1
#define DD_ALIGN_EVENT_DEL 2
#define DD_ALIGN_EVENTS_MAX_CAP 4096
/* Device pointers.  Reads what the dd_align_haplotypes_device launch of b_dev / r_dev left in r_dev->status and r_dev->ref_pos and writes
 * per pair n_events_dev[pair] (the true count, also when it exceeds events_cap; 0 for a pair whose status is not DD_ALIGN_OK) and the
 * first min(count, events_cap) records of events_dev[pair * events_cap ...]; nothing else of events_dev is written.  It runs BEHIND
 * dd_align_haplotypes_device: same host thread, same stream, that launch's workspace still allocated — its pair counter and guard words
 * live in that workspace's header (DD_ERR_INVALID when this thread has launched no alignment).  events_cap 1 ... DD_ALIGN_EVENTS_MAX_CAP.
 * Asynchronous on `stream`, no allocation. */
int dd_align_events_device(const dd_align_batch *b_dev, const dd_align_result *r_dev, int32_t *n_events_dev, dd_align_events *events_dev,
                           int events_cap, void *stream);
/* Host pointers: dd_align_haplotypes followed by the event launch.  score, status, n_events [n_pairs] and events [n_pairs * events_cap]
 * always come back; r->ref_pos may be NULL, then no slice is copied back (the point of this entry: 8 * events_cap + 12 bytes per pair
 * instead of two per haplotype base).  A pair with n_events > events_cap holds its first events_cap records; the caller redoes it from
 * the slice.  Validation and errors as dd_align_haplotypes. */
int dd_align_haplotypes_events(const dd_align_batch *b, dd_align_result *r, int32_t *n_events, dd_align_events *events, int events_cap,
                               int device);
/* The last event launch on this host thread: {grid (workgroups), pairs, most pairs one wavefront drew, wavefronts stopped by the draw
 * guard}; the last two as in dd_align_last_launch (0 is the only healthy guard count). */
#define DD_ALIGN_EVENTS_LOG_FIELDS 4
void dd_align_events_last_launch(int64_t out[DD_ALIGN_EVENTS_LOG_FIELDS]);

/* ---- variants of an alignment: everything convertAlignment and getFlankingCoordinatesBetter give per haplotype, without strings ---- */
/* One variant of one pair, in column order (reference ObservationModelSeqAn.hpp:37-269).  Strings are not produced: the caller forms
 * "+...", "-...", "X=>X" from the two sequences by position.
 *   kind        DD_ALIGN_EVENT_INS, DD_ALIGN_EVENT_DEL, DD_HAP_VARIANT_SNP, or DD_HAP_VARIANT_DEL_UNSEEN: deleted reference bases in
 *               front of the first paired base, which convertAlignment marks 'D' in hap.align but does not record as a variant
 *   key         the map key (hb): reference bases left of the variant
 *   len         inserted haplotype bases / deleted reference bases / 1
 *   start_read  AlignedVariant::startRead: first inserted base; the base in front of a deletion; the SNP's base
 *   left_flank_hap ... right_flank_read   the four arguments of AlignedVariant::setFlanking, in its order (0 for DEL_UNSEEN, and for
 *               an insertion that raised DD_HAP_VARIANTS_HOST)
 * The classification rules are those of dd_align_events, a SNP being a paired base whose seqan::Dna letter differs from the reference
 * base's.  Records of a later column come later; a deletion in front of base b comes before what base b itself gives.  Two records
 * may carry one key (an insertion, then a deletion that starts behind it): the later one replaces the earlier in hap.indels.
 * No field truncates: sequences are at most DD_LONG_MAX_HAP_LEN = 4,094 bases, so key, len, start_read and the haplotype flanks are
 * at most 4,094 and the read flanks, sums of a read position and a difference of reference positions, at most 8,188 and never
 * negative (getFlankingCoordinatesBetter clamps the left one at 0 and start_read of a recorded deletion is at least 0). */
typedef struct dd_hap_variant {
    int16_t kind, key, len, start_read, left_flank_hap, right_flank_hap, left_flank_read, right_flank_read;
} dd_hap_variant;
#define DD_HAP_VARIANT_SNP 3
#define DD_HAP_VARIANT_DEL_UNSEEN 4
/* Per pair.  n_variants: the true number of records, also beyond the launch's cap.  first_base / last_base: ml.firstBase (-1: no paired
 * base) and ml.lastBase as convertAlignment leaves them.  flags: DD_HAP_VARIANTS_* .  A pair whose status is not DD_ALIGN_OK has all
 * four 0 and no records. */
typedef struct dd_hap_variants_summary {
    int32_t n_variants, first_base, last_base, flags;
} dd_hap_variants_summary;
#define DD_HAP_VARIANTS_LO_FIRST 1   /* haplotype base 0 is MLAlignment::LO */
#define DD_HAP_VARIANTS_RO_LAST  2   /* the last haplotype base is MLAlignment::RO and the haplotype has more than one base */
#define DD_HAP_VARIANTS_HOST     4   /* a flank of this pair has no closed form (an insertion at least as long as the reference sequence):
                                        convert the pair on the host from its slice */
#define DD_HAP_VARIANTS_MAX_CAP 4096
/* Device pointers; runs BEHIND dd_align_haplotypes_device exactly like dd_align_events_device (same thread, same stream, that launch's
 * workspace still allocated: header words of its own).  Writes summary_dev[pair] for every pair and the first min(n_variants, cap)
 * records of variants_dev[pair * cap ...] (8-byte aligned); nothing else of variants_dev is written.  Reads both sequences of b_dev.
 * cap 1 ... DD_HAP_VARIANTS_MAX_CAP.  Asynchronous on `stream`, no allocation. */
int dd_hap_variants_device(const dd_align_batch *b_dev, const dd_align_result *r_dev, dd_hap_variants_summary *summary_dev,
                           dd_hap_variant *variants_dev, int cap, void *stream);
/* Host pointers: dd_align_haplotypes followed by the variants launch.  score, status, summary [n_pairs] and variants [n_pairs * cap]
 * always come back (records the kernel did not write are 0); r->ref_pos may be NULL, then no slice is copied back.  Validation and
 * errors as dd_align_haplotypes. */
int dd_align_haplotypes_variants(const dd_align_batch *b, dd_align_result *r, dd_hap_variants_summary *summary, dd_hap_variant *variants,
                                 int cap, int device);
/* The last variants launch on this host thread: the fields of dd_align_events_last_launch. */
void dd_hap_variants_last_launch(int64_t out[DD_ALIGN_EVENTS_LOG_FIELDS]);

/* ---- block table of a window's empirical haplotype distribution (HaplotypeDistribution / HapBlock) ---------- */
/* Windows and the reads laid over them, CSR-packed.  Raw addresses: host arrays for dd_hap_blocks_compute, device arrays for
 * dd_hap_blocks_device.  A window is the reference piece [rs, rs + len) (len = win_ref_off[w + 1] - win_ref_off[w], the bytes as
 * getRefSeq returned them) and the reads win_read_off[w] ... win_read_off[w + 1], in getReads' order.  A read is its 0-based position,
 * its BAM flag, its CIGAR as BAM words (len << 4 | op) and its bases as letters (=ACMGRSVTWYHKDBN). */
typedef struct dd_hap_batch {
    int32_t n_windows;
    const int32_t *win_rs;            /* [n_windows] */
    const int32_t *win_ref_off;       /* [n_windows + 1], starts at 0 */
    const char *ref_seq;
    const int32_t *win_read_off;      /* [n_windows + 1], starts at 0 */
    int32_t n_reads;
    const int32_t *read_pos;          /* [n_reads] */
    const int32_t *read_flag;         /* [n_reads] */
    const int32_t *read_op_off;       /* [n_reads + 1], starts at 0 */
    const uint32_t *ops;
    const int32_t *read_base_off;     /* [n_reads + 1], starts at 0 */
    const char *bases;
} dd_hap_batch;
/* Per-window status.  A window whose status is not DD_HAPDIST_OK has nothing but its status written. */
#define DD_HAPDIST_OK 0
#define DD_HAPDIST_TOO_WIDE 1         /* the reference piece is longer than DD_HAPDIST_MAX_WINDOW */
#define DD_HAPDIST_OVERFLOW 2         /* a block with more than DD_HAPDIST_MAX_DISTINCT strings, more than DD_HAPDIST_MAX_INS_POS insertion
                                       * positions, or more blocks / entries / insertions than the window's capacity in dd_hap_blocks */
#define DD_HAPDIST_HOST 3             /* the reference throws on this window (an operation it does not know, "Mag niet."), or the input is one
                                       * the closed form does not cover (empty reference piece, negative position with operations, a CIGAR
                                       * longer than its read's bases): the caller runs its literal path */
#define DD_HAPDIST_MAX_WINDOW 1024
#define DD_HAPDIST_MAX_DISTINCT 16
#define DD_HAPDIST_MAX_INS_POS 64
/* The tables.  Capacities are the caller's: window w owns blocks[blk_off[w] ... blk_off[w + 1]), entries[ent_off[w] ... ent_off[w + 1])
 * and ins_ops / ins_pos[ins_off[w] ... ins_off[w + 1]); dd_hap_blocks_offsets fills the three offset arrays with capacities no OK window
 * can exceed except through DD_HAPDIST_OVERFLOW.  Raw addresses like dd_hap_batch.
 *   blocks   one word per block inside the window, in position order: start - rs (bits 0-15), length 1 ... 4 (16-19), entries (20-25),
 *            index of the entry equal to the reference piece (26-31)
 *   entries  two words per entry, blocks back to back, a block's entries in std::string order: key (the bytes big-endian, left-aligned),
 *            count (covering segments that show it; the reference counts once)
 *   ins_ops  two words per insertion operation (length > 0) that starts inside the window, in (read, operation) order: read index inside the
 *            window, operation index << 16 | (position - rs)
 *   ins_pos  two words per insertion position in order of creation: position - rs, and what the empty (reference) entry collected from
 *            operations crossing the position after its creation (its count is that + 1)
 *   left     bit 0: a segment covers rs - 1 (the block left of the window ends there); bit 1: a segment starts left of rs */
typedef struct dd_hap_blocks {
    int32_t *status, *n_blocks, *n_entries, *n_ins_ops, *n_ins_pos, *left;   /* [n_windows] each */
    const int32_t *blk_off, *ent_off, *ins_off;                              /* [n_windows + 1] each, start at 0 */
    uint32_t *blocks, *entries, *ins_ops, *ins_pos;
} dd_hap_blocks;
/* Host pointers, no device: blk_off / ent_off / ins_off [n_windows + 1] for a batch (blocks: the window's length; entries: 4 per position
 * + 64; insertions: the insertion operations of the window's reads). */
int dd_hap_blocks_offsets(const dd_hap_batch *b, int32_t *blk_off, int32_t *ent_off, int32_t *ins_off);
/* Bytes of the workspace dd_hap_blocks_device needs (the window counter and the draw guard's words). */
size_t dd_hap_blocks_workspace_bytes(void);
/* Device pointers, any stream, no allocation.  The offsets are checked on the device against nothing but themselves: max_blk, max_ent
 * and max_ins are the lengths of blocks, entries / 2 and ins_ops / 2 = ins_pos / 2 the caller allocated, and no store goes past them. */
int dd_hap_blocks_device(const dd_hap_batch *b_dev, const dd_hap_blocks *t_dev, int64_t max_blk, int64_t max_ent, int64_t max_ins,
                         void *workspace, size_t workspace_bytes, void *stream);
/* Host pointers: validates, copies, launches, copies back.  DD_ERR_INVALID before any launch; DD_ERR_NO_DEVICE without a GPU. */
int dd_hap_blocks_compute(const dd_hap_batch *b, dd_hap_blocks *t, int device);
/* The last block-table launch on this host thread: {grid (workgroups), windows, most windows one wavefront drew, wavefronts stopped by the
 * draw guard}; the last two as in dd_align_last_launch (0 is the only healthy guard count). */
#define DD_HAP_BLOCKS_LOG_FIELDS 4
void dd_hap_blocks_last_launch(int64_t out[DD_HAP_BLOCKS_LOG_FIELDS]);

/* ---- N1 (next row): read sums of the diploid genotype reduction --------------------------- */
/* S[w][h1*H_w+h2] (h1<=h2) = sum over the window's reads, in order, of log(0.5)+addLogs(ll[h1][r], ll[h2][r])
 * — the inner loop of DetInDel::diploidGLF, reference DInDel.cpp:3085-3091 (and :3372-3374); addLogs is
 * reference Utils.hpp:29-38.  `ll` is the per-pair array dd_launch_device / dd_compute_likelihoods produced.
 * win_hh_off[n_windows+1] = prefix sums of H_w^2 (dd_pair_sum_offsets).  exp/log run on the device:
 * agreement with glibc is ~1e-15 relative, not bit-for-bit. */
int dd_pair_sum_offsets(const dd_batch *b, int64_t *win_hh_off);
int dd_pair_sums_device(const dd_device_batch *b, const int64_t *win_hh_off_dev, int64_t n_slots,
                        const double *ll_dev, double *out_dev, void *stream);
int dd_pair_sums(const dd_batch *b, const double *ll_host, double *out_host, int device);

/* MAP haplotype pairs of the same function (reference DInDel.cpp:3073-3118), per window, on the device:
 *   posterior[h1*H+h2] = S[h1,h2] + prior[h1,h2] for h1<=h2 with filtered[h1]==filtered[h2]==0 (0 elsewhere)     (:3091)
 *   pairs[4w+0..1] = first strict maximum among pairs with ncand[h1]>0 || ncand[h2]>0  (max_indel_pair, -1 if none) (:3103)
 *   pairs[4w+2..3] = the same among pairs with no candidate indel (max_noindel_pair)                                (:3108)
 *   vals[3w+0..2]  = max_ll_indel, max_ll_noindel (= ll_ref), qual = -10 (ll_ref - addLogs(max_ll_indel, ll_ref)) / ln 10 (:3116-3118)
 * prior = DetInDel::getHaplotypePrior per pair (:3064-3068, host data), filtered[n_haps] from filterHaplotypes (:2941),
 * ncand[n_haps] = hap_num_candidate_indels (:2984-2993).  The caller raises the reference's
 * `throw string("Could not find indel allele")` (:3121) when pairs[4w] == -1.
 * dd_map_pairs: host pointers; runs the read sums (from `ll`) and this step in one go; pair_sum_out / posterior_out may be NULL. */
int dd_map_pairs_device(const dd_device_batch *b, const int64_t *win_hh_off_dev, const double *pair_sum_dev,
                        const double *prior_dev, const uint8_t *filtered_dev, const int32_t *ncand_dev,
                        double *posterior_dev, int32_t *pairs_dev, double *vals_dev, void *stream);
int dd_map_pairs(const dd_batch *b, const double *ll_host, const double *prior_host, const uint8_t *filtered_host,
                 const int32_t *ncand_host, double *pair_sum_out, double *posterior_out, int32_t *pairs_out,
                 double *vals_out, int device);

/* ---- pooled analysis: the EM loop of estimateHaplotypeFrequenciesBayesEM (reference DInDel.cpp:2412-2543) ---------- */
/* A slot is one (window, set of active variants): the loop runs once per slot over the window's `ll` (rl[r,h] = ll[pair(w,h,r)]) with the
 * haplotypes the set is compatible with (:2393-2408, the caller's).  The arithmetic is csrc/pooled_math.h on the host and on the device:
 * fp64 operations and series of its own, one order of every sum (read r in partial r mod 64, partials combined pairwise from 32 down),
 * so every output of the three entries below is the same in every bit.  It is not the reference's libm / Boost arithmetic; DESIGN 20
 * gives its error against exact arithmetic.
 *   slot_window [n_slots]          window of the slot
 *   slot_off    [n_slots + 1]      starts at 0; slot s owns compat / freqs [slot_off[s], slot_off[s + 1]), as many as its window has haplotypes
 *   compat                         one byte per (slot, haplotype), 0 = incompatible (lpi = pi = -100)
 * Outputs per slot: loglik (the last iteration's), freqs (exp(pi) normalised), iters (iterations run, at most 27; -1 on the device when
 * the slot's tables do not fit its window or max_haps), ediff (the last |eOld - eNew|).  Raw addresses: host or device arrays. */
typedef struct dd_pooled_slots {
    int64_t n_slots;
    const int32_t *slot_window;
    const int64_t *slot_off;
    const uint8_t *compat;
} dd_pooled_slots;
typedef struct dd_pooled_result {
    double *loglik;                   /* [n_slots] */
    double *freqs;                    /* [slot_off[n_slots]] */
    int32_t *iters;                   /* [n_slots] */
    double *ediff;                    /* [n_slots] */
} dd_pooled_result;
/* Device pointers, on a stream, behind any likelihood launch; asynchronous, no allocation.  Of the batch it reads n_windows, win_hap_off,
 * win_read_off and win_pair_off.  max_haps: the most haplotypes a window of the batch has (the launch's LDS is sized from it, 536 bytes
 * per haplotype; at most DD_POOLED_MAX_HAPS).  a0 > 0: the Dirichlet parameter (--bayesa0); tol: EMtol. */
#define DD_POOLED_MAX_HAPS 256
int dd_pooled_em_device(const dd_device_batch *b, const double *ll_dev, const dd_pooled_slots *s_dev, int max_haps, double a0, double tol,
                        const dd_pooled_result *out_dev, void *stream);
/* Host pointers: validates, copies, launches, copies back.  DD_ERR_INVALID before any launch; DD_ERR_NO_DEVICE without a GPU. */
int dd_pooled_em(const dd_batch *b, const double *ll_host, const dd_pooled_slots *s, double a0, double tol, const dd_pooled_result *out,
                 int device);
/* The same loop on the CPU, no device needed: slots spread over nthreads host threads (< 1: one). */
int dd_pooled_em_host(const dd_batch *b, const double *ll_host, const dd_pooled_slots *s, double a0, double tol, const dd_pooled_result *out,
                      int nthreads);
/* pooled_math.h's functions over an array (host): fn 0 = exp, 1 = log, 2 = digamma; fn 3 = addLogs over pairs x[2i], x[2i + 1]. */
int dd_pooled_math_eval(int fn, const double *x, double *y, int64_t n);

/* ---- the --faster model's indel-map key count on the device (opt-in) ------------------------ */
/* The --faster model (ObservationModelS) leaves dd_result.numIndels 0; what the reference's window loop reads per pair is
 * liks[h][r].indels.size() (DInDel.cpp:3529), the number of DISTINCT keys reportVariants enters into the record's indel map
 * (Faster.cpp:553-661).  That number follows from the pair's hpos alone (csrc/indel_keys_kernel.h is the definition):
 *     lhp = 1; walk b upward from 0.  hp[b] inserted (DD_HPOS_IS_INS): take the maximal run of such entries; with c its first entry the
 *     key is DD_HPOS_INS_POS(c), or lhp when c is the bare DD_HPOS_INS; continue behind the run.  Otherwise, with c = hp[b]: c >= 0 sets
 *     lhp = c + 1, and if also b < L-1, hp[b+1] >= 0 and hp[b+1] - c > 1 the key is c + 1; then b++.
 * Computed on the device from the hpos the likelihood kernels left there, 2 bytes per pair come back instead of the pair's 2 L bytes of
 * hpos.  One int16 per pair, in pair order: the count when it is at most DD_INDEL_KEYS_CAP, DD_INDEL_KEYS_OVERFLOW when there are more
 * distinct keys, DD_INDEL_KEYS_NOT_COMPUTED for a pair whose dd_result.status is not DD_PAIR_OK (its hpos is not read).  Any int16
 * content of hpos gives the same answer on the device and on the host. */
#define DD_INDEL_KEYS_CAP           64
#define DD_INDEL_KEYS_OVERFLOW      (-1)
#define DD_INDEL_KEYS_NOT_COMPUTED  (-2)
/* Enqueue the launch for the whole batch on `stream`, behind the likelihood launch(es) that wrote hpos_dev and status_dev (any of them:
 * hpos is only read).  DEVICE pointers: hpos_dev (dd_result.hpos), status_dev (dd_result.status; NULL = every pair was computed), out_dev
 * (int16 [n_pairs]).  Of the batch it reads n_windows, n_haps, n_reads, win_read_off, read_seq_off, win_pair_off and win_hpos_off.
 * Asynchronous, no allocation, no synchronisation. */
int dd_indel_keys_device(const dd_device_batch *b, const int16_t *hpos_dev, const int32_t *status_dev, int16_t *out_dev, void *stream);
/* The same values on the CPU from host arrays, no device needed: pairs spread over nthreads host threads (< 1: one).  Of the batch it
 * reads n_windows and the four offset arrays (win_hap_off, win_read_off, hap_seq_off, read_seq_off). */
int dd_indel_keys_host(const dd_batch *b, const int16_t *hpos_host, const int32_t *status_host, int16_t *out, int nthreads);
/* Host pointers: dd_compute_likelihoods_faster_ex (options: 0 or DD_OPT_LONG_WINDOWS_FASTER) with, per window block, the key launch behind
 * the block's likelihood launches; keys_out (int16 [n_pairs], host memory) is filled.  r->hpos may be NULL: the per-base alignments then
 * stay on the device — the point of this entry.  Everything else as dd_compute_likelihoods_faster_ex. */
int dd_compute_likelihoods_faster_keys(const dd_params *p, const dd_batch *b, dd_result *r, int16_t *keys_out, int device, uint32_t options);

/* ---- audit: a sample of a launch's windows recomputed by the long-window kernel and compared on the device (opt-in) ---------- */
/* The main model has two implementations in this library: the main kernels (hmm_kernel.hip, one build per
 * haplotype-length class and maxLengthDel) and the long-window kernel (long_kernel.hip: one workgroup per pair, a run-time candidate loop,
 * no speculative skip; no kernel text in common with hmm_kernel.hip, though it includes hmm_kernel.h and kernel_common.h for the table
 * layout and the symbol codes and reads the same tables and symbol LUT), which takes any haplotype of 1..DD_LONG_MAX_HAP_LEN bp and any
 * maxLengthDel.  An audit recomputes a seeded sample
 * of a launch's DD_WIN_MAIN windows with the long-window kernel into shadow buffers as large as the sample and compares them, bit for bit
 * and on the device, with what the main kernels left in HBM.  It shows that two independently compiled kernels agree on the sample; it
 * does not prove a launch right.  Main model only (the --faster model's long kernel shares its main kernel's text: that model is audited
 * against a shadow kernel of its own, "audit of the --faster model" below).  Without these entries nothing changes.
 *
 * What is compared for one audited pair (csrc/audit_kernel.h is the definition, shared by the kernel and dd_audit_compare_host):
 *   status first; if the two differ that is ONE difference (DD_AUDIT_FIELD_status) and nothing else of the pair is compared
 *   DD_PAIR_OK, _NAN, _LLPOS   every per-pair value (ll ... lastBase), the pair's L entries of hpos, its var_covered bytes, and its
 *                              var_fcov bytes when the batch has hap_var_flank
 *   DD_PAIR_HAPSIZE            ll, var_covered, and var_fcov when the batch has hap_var_flank
 *   any other status           nothing more
 *   onHap is derived and never compared; a field whose pointer is NULL on either side is skipped; equality is equality of bits (doubles
 *   as 64-bit integers: NaNs and signed zeros count); an element the rule does not name is never read, on either side. */
enum {
    DD_AUDIT_FIELD_status = 0, DD_AUDIT_FIELD_ll, DD_AUDIT_FIELD_llOn, DD_AUDIT_FIELD_llOff, DD_AUDIT_FIELD_mLogBQ, DD_AUDIT_FIELD_offHap,
    DD_AUDIT_FIELD_offHapHMQ, DD_AUDIT_FIELD_numIndels, DD_AUDIT_FIELD_numMismatch, DD_AUDIT_FIELD_nBQT, DD_AUDIT_FIELD_nmmBQT,
    DD_AUDIT_FIELD_nMMLeft, DD_AUDIT_FIELD_nMMRight, DD_AUDIT_FIELD_firstBase, DD_AUDIT_FIELD_lastBase, DD_AUDIT_FIELD_hpos,
    DD_AUDIT_FIELD_var_covered, DD_AUDIT_FIELD_var_fcov, DD_AUDIT_N_FIELDS
};
/* One difference.  index: the element's index in the PRIMARY array (the pair for a per-pair value); the bits are zero-extended. */
typedef struct dd_audit_record {
    int32_t  window, field;
    int64_t  pair, index;
    uint64_t primary_bits, shadow_bits;
} dd_audit_record;
/* A report: this header, then max_records records.  n_diff counts every difference, also beyond max_records; the first
 * min(n_diff, max_records) records are written, in any order; the other record slots are zero. */
typedef struct dd_audit_report {
    int64_t n_pairs;                        /* pairs compared */
    int64_t n_diff;                         /* differences found = sum of diff[] */
    int64_t diff[DD_AUDIT_N_FIELDS];        /* differences per field */
    int64_t compared[DD_AUDIT_N_FIELDS];    /* elements compared per field (status: one per pair) */
} dd_audit_report;
#define DD_AUDIT_REPORT_BYTES(max_records) (sizeof(dd_audit_report) + (size_t)(max_records) * sizeof(dd_audit_record))
/* The shadow of a sample: what its result arrays must hold, and what the long launch is planned for. */
typedef struct dd_audit_sizes {
    int32_t n_windows;                      /* chosen windows */
    int32_t max_hap_len, max_read_len;      /* longest haplotype / read among them (0: none chosen) */
    int32_t reserved;
    int64_t n_pairs, hpos_len, var_cov_len; /* elements of the shadow's per-pair arrays, of its hpos, bytes of each coverage array */
} dd_audit_sizes;
/* Choose the sample (host arithmetic, no device).  Eligible: windows of class DD_WIN_MAIN (win_class: dd_screen_windows_ex's or
 * dd_screen_windows' bytes; NULL = every window) with at least one pair, no empty read or haplotype and nothing beyond the long limits.
 * The choice is a function of (seed, batch, win_class, p, n_want) alone: when n_want is at least the number of launch classes of
 * dd_build_length_classes that hold a haplotype of an eligible window, every such class gets a chosen window that holds one of its
 * haplotypes (one kernel build serves one class, so every build the launch selects is audited); the rest is drawn uniformly from the
 * eligible windows not yet chosen.  n_want <= 0 chooses none, n_want at or above the eligible count all.
 *   audit_class [n_windows]       DD_WIN_LONG for a chosen window, DD_WIN_UNSUPPORTED elsewhere
 *   pair_off, hpos_off, varcov_off [n_windows + 1]   where window w starts in the shadow: prefix sums of dd_batch_offsets' differences over
 *                                 the chosen windows alone (another window has width 0 there)
 * Returns the number of eligible windows (>= 0) or a DD_ERR_* code. */
int dd_audit_select(const dd_params *p, const dd_batch *b, const uint8_t *win_class, uint64_t seed, int32_t n_want, uint8_t *audit_class,
                    int64_t *pair_off, int64_t *hpos_off, int64_t *varcov_off, dd_audit_sizes *sizes);
/* dd_audit_select's outputs where the comparison runs: DEVICE copies for dd_audit_device, the host arrays for dd_audit_compare_host.
 * n_windows and n_qual are the batch's. */
typedef struct dd_audit_view {
    int32_t n_windows, n_qual;
    const uint8_t *audit_class;
    const int64_t *pair_off, *hpos_off, *varcov_off;
    dd_audit_sizes sizes;
} dd_audit_view;
/* Bytes of device workspace dd_audit_device needs: the long launch's for the sample's maxima (dd_workspace_bytes_long's layout).  0 when
 * nothing is chosen or a shape is beyond the long limits.  Never shared by two launches that may run at the same time. */
size_t dd_audit_workspace_bytes(const dd_params *p, const dd_audit_view *view);
/* Enqueue the audit on `stream`, behind the likelihood launch(es) that wrote `primary` (dd_launch_device, and dd_launch_device_long when
 * the batch has long windows): the long-window launch over the chosen windows into `shadow` (DEVICE arrays of view->sizes' lengths; ll and
 * status required, onHap ignored), then the comparison (audit_kernel.hip) into report_dev (DD_AUDIT_REPORT_BYTES(max_records) bytes of
 * device memory, 8-byte aligned; zeroed on the stream first).  `primary` is only read; b is the batch of the likelihood launch, as it was
 * handed to it.  Asynchronous; no allocation, no synchronisation.  DD_ERR_NO_DEVICE without a GPU: there is no CPU fallback behind this
 * entry. */
int dd_audit_device(const dd_params *p, const dd_device_batch *b, const dd_result *primary, const dd_audit_view *view, const dd_result *shadow,
                    void *report_dev, int64_t max_records, void *workspace, size_t workspace_bytes, void *stream);
/* The audit's long launch of the last dd_audit_device / dd_compute_likelihoods_audit call on this host thread (the last window block's, for
 * the latter): {grid of the long launch, pairs recomputed, most pairs one workgroup took, workspace bytes, K (states per thread / 256),
 * the sample's longest haplotype, longest read, grid of the comparison}; all 0 when nothing was launched.  The two counters are read from
 * the workspace header (or the host path's own copy): this synchronises the stream, and after dd_audit_device the workspace must still
 * be allocated (-1 if the read fails).  dd_long_launch_log is not touched by an audit. */
#define DD_AUDIT_LOG_FIELDS 8
void dd_audit_last_launch(int64_t out[DD_AUDIT_LOG_FIELDS]);
/* The same comparison on the CPU from host arrays, no device needed: `view` holds dd_audit_select's host arrays, `shadow` host arrays of
 * view->sizes' lengths, `report` DD_AUDIT_REPORT_BYTES(max_records) bytes.  Records come in pair order, a pair's in field order. */
int dd_audit_compare_host(const dd_batch *b, const dd_result *primary, const dd_audit_view *view, const dd_result *shadow, void *report,
                          int64_t max_records);
/* Host pointers: dd_compute_likelihoods_ex (options: 0 or DD_OPT_LONG_WINDOWS) with an audit of n_want windows of the batch, chosen once
 * with `seed` (dd_audit_select over the whole batch): every window block audits its own chosen windows on its own stream, behind its
 * likelihood launches and in front of its copy back.  report: DD_AUDIT_REPORT_BYTES(max_records) bytes of host memory; its counts are the
 * sums over the blocks, its records the first max_records differences of all blocks, in any order.  r comes back exactly as from
 * dd_compute_likelihoods_ex.  A batch without pairs, and n_want <= 0, give an empty report. */
int dd_compute_likelihoods_audit(const dd_params *p, const dd_batch *b, dd_result *r, int device, uint32_t options, uint64_t seed,
                                 int32_t n_want, void *report, int64_t max_records);

/* TEST HOOK, not for production callers: the next dd_compute_likelihoods_audit (or dd_compute_likelihoods_faster_audit, below) call of this
 * host thread inverts the lowest bit of the
 * device copy of ll of `window`'s first pair in front of that window's audit and restores it behind it (also when the audit's launch
 * fails), so that the caller's results are not affected; the call synchronises the window block's stream once to read the value.  A
 * window the audit did not choose, or without pairs: nothing happens.  -1 = none.  It lets a caller's handling of a difference be tested
 * without anything going wrong on the device (dindel_gpu --auditInject). */
void dd_audit_inject_next(int window);

/* ---- audit of the --faster model: a sample of a --faster launch's windows recomputed by an independent shadow kernel (opt-in) -------- */
/* The --faster model's two kernels (faster_kernel.hip, faster_long_kernel.hip) are one text, so neither can check the other.  These
 * entries recompute a seeded sample of a --faster launch's windows with a second implementation of ObservationModelS, written from the
 * reference and not from those kernels (csrc/faster_shadow.h: one function per destination state, shared by the shadow kernel
 * faster_shadow_kernel.hip — one wavefront per pair — and the CPU evaluation below), and compare bit for bit on the device.  As above, an
 * audit shows that two independently compiled kernels agree on the sample, not that a launch is right.  What the shadow shares with the
 * kernels it checks, and so cannot see: dd_build_tables' block and its layout, the index arrays and the batch, and the rule itself.
 *
 * The rule for this model (au_compared_faster in csrc/faster_shadow.h), where it differs from the main model's:
 *   DD_PAIR_OK                      every per-pair value, the pair's L entries of hpos, var_covered, and var_fcov with hap_var_flank
 *   DD_PAIR_NAN, DD_PAIR_HAPSIZE    ll (0), llOn ... nMMRight (the eleven fields the model leaves at defaults; offHapHMQ = 1), var_covered,
 *                                   var_fcov with hap_var_flank; NOT firstBase, lastBase, hpos: the kernels never write them for such a pair
 * Records, report, field ids, views and sizes are the main model's audit's. */
/* dd_audit_select for a --faster launch.  Eligible: windows of class DD_WIN_MAIN of the --faster screen (win_class:
 * dd_screen_windows_ex's bytes with DD_OPT_LONG_WINDOWS_FASTER, or dd_screen_windows'; NULL = every window) with at least one pair, and,
 * when `options` has DD_OPT_LONG_WINDOWS_FASTER, those of class DD_WIN_LONG as well (the shadow is independent of the long kernel too);
 * never a window with an empty read or haplotype or a shape beyond the long limits.  When n_want allows (>= the number of them) the sample
 * first takes the window holding the longest ordinary haplotype (<= DD_MAX_HAP_LEN bp), the one holding the longest ordinary read
 * (<= DD_MAX_READ_LEN bp) — the two shapes the --faster launch sizes its LDS for; lowest window index on a tie — and one long window if any
 * is eligible (drawn with the seed); the rest is the same seeded partial shuffle.  A pure function of its arguments.  Outputs and return
 * value as dd_audit_select. */
int dd_audit_select_faster(const dd_params *p, const dd_batch *b, const uint8_t *win_class, uint32_t options, uint64_t seed, int32_t n_want,
                           uint8_t *audit_class, int64_t *pair_off, int64_t *hpos_off, int64_t *varcov_off, dd_audit_sizes *sizes);
/* Bytes of device workspace dd_audit_device_faster needs: 0 while the sample's longest haplotype and read are ordinary (the shadow
 * kernel's back-pointer tile and vote histogram are then in LDS), else one area per wavefront of its grid, the grid shrunk to keep the
 * total within 256 MiB.  Never shared by two launches that may run at the same time. */
size_t dd_audit_workspace_bytes_faster(const dd_params *p, const dd_audit_view *view);
/* Enqueue the audit on `stream`, behind dd_launch_device_faster (and dd_launch_device_faster_long where the batch has long windows) that
 * wrote `primary`: the shadow kernel over the sample into `shadow` (DEVICE arrays of view->sizes' lengths; ll and status required, onHap
 * ignored), then the comparison into report_dev (as dd_audit_device's).  `primary` is only read.  workspace may be NULL when
 * dd_audit_workspace_bytes_faster is 0.  Asynchronous; no allocation, no synchronisation.  DD_ERR_NO_DEVICE without a GPU. */
int dd_audit_device_faster(const dd_params *p, const dd_device_batch *b, const dd_result *primary, const dd_audit_view *view,
                           const dd_result *shadow, void *report_dev, int64_t max_records, void *workspace, size_t workspace_bytes, void *stream);
/* The shadow launch of the last dd_audit_device_faster call on this host thread: {grid of the shadow kernel, pairs recomputed, 1 if its
 * areas were in LDS else 0, workspace bytes, LDS bytes per workgroup, the sample's longest haplotype, longest read, grid of the
 * comparison}; all 0 when nothing was launched.  Host-side values only: nothing is read from the device. */
void dd_audit_last_launch_faster(int64_t out[DD_AUDIT_LOG_FIELDS]);
/* The shadow on the CPU, no device needed: the same functions the shadow kernel calls (csrc/faster_shadow.h), looped over the sample's
 * pairs and their destination states.  view: dd_audit_select_faster's host arrays; shadow: host arrays of view->sizes' lengths (ll and
 * status required; NULL fields are not written).  Writes exactly the elements the rule names for each pair's status. */
int dd_audit_shadow_faster_host(const dd_params *p, const dd_batch *b, const dd_audit_view *view, const dd_result *shadow);
/* dd_audit_compare_host under this model's rule. */
int dd_audit_compare_host_faster(const dd_batch *b, const dd_result *primary, const dd_audit_view *view, const dd_result *shadow, void *report,
                                 int64_t max_records);
/* Host pointers: dd_compute_likelihoods_faster_ex (options: 0 or DD_OPT_LONG_WINDOWS_FASTER) with an audit of n_want windows of the batch,
 * chosen once with `seed` (dd_audit_select_faster over the whole batch, with the same options): every window block audits its own chosen
 * windows on its own stream, behind its --faster launches and in front of its copy back.  keys_out may be NULL; when given (one int16 per
 * pair) the key launch runs per block as in dd_compute_likelihoods_faster_keys, and hpos — then on the device whether r->hpos is given or
 * not — is compared: the configuration --faster is run in.  report, max_records, the empty report and the caller's results: as
 * dd_compute_likelihoods_audit; r (and keys_out) come back exactly as from the call without audit.  dd_audit_inject_next applies to this
 * entry too.  dd_audit_last_launch_faster then describes the last window block's shadow launch. */
int dd_compute_likelihoods_faster_audit(const dd_params *p, const dd_batch *b, dd_result *r, int16_t *keys_out, int device, uint32_t options,
                                        uint64_t seed, int32_t n_want, void *report, int64_t max_records);

/* Launch plan the library would use for the main kernel on a batch with these maxima (no device needed):
 * out = {K positions per lane, D build (6 / 11 / 12), 1 if back-pointers go to HBM scratch else 0, waves per workgroup,
 *        read split of a haplotype, LDS bytes per workgroup, scratch bytes (low 31 bits, in KiB), waves per CU the plan expects,
 *        pairs per wavefront (1, or 2: the builds that run two reads side by side on 32-lane halves), 0}.
 * avg_reads = reads per window, n_haps = haplotypes the launch covers. */
int dd_plan_info(const dd_params *p, int max_hap_len, int max_read_len, int n_qual, int avg_reads, int n_haps, int32_t out[10]);

/* name of the dominant kernel as rocprofv3 reports it, and launch geometry of the last launch */
const char *dd_kernel_name(void);
/* geometry of the last dd_launch_device on this host thread's library instance:
 * {K positions/lane, D build, waves/workgroup, LDS bytes/workgroup, grid, read split, LDS bytes/wave, shared LDS bytes} */
void dd_last_launch(int32_t out[8]);
/* Every main-model kernel launch of the last dd_launch_device / dd_compute_likelihoods call on this host thread (a ragged batch is one
 * launch per non-empty (haplotype class, read class)): up to max_records records of DD_LAUNCH_LOG_FIELDS int32 each are written to out,
 * the number of launches is returned.  Record: {K positions per lane, pairs per wavefront (1, or 2 on 32-lane halves), D build,
 * 1 = back-pointers in HBM scratch, 1 = FOLD build, waves per workgroup, LDS bytes per workgroup, grid, read split, haplotypes covered,
 * longest haplotype of the class, shortest admissible read, longest read of the class, waves per CU the plan expects, occupancy variant,
 * duration in microseconds (-1 unless the process runs with DD_LAUNCH_TIMING=1: diagnostics, the read-out synchronises),
 * 1 = persistent grid drawing its items from a counter (ragged launches), reads per wavefront a haplotype's workgroups are sized for (0 = the
 * launch's read split for every haplotype)}. */
#define DD_LAUNCH_LOG_FIELDS 18
int dd_launch_log(int32_t *out, int max_records);
/* How many output arrays of the last dd_compute_likelihoods / _faster call on this host thread were written by the kernels directly
 * into the caller's memory: arrays that lie in page-locked, device-addressable host memory (dd_host_alloc, hipHostMalloc) are
 * not staged in HBM and not copied afterwards (status and offHapHMQ excepted).  0 for pageable memory. */
int dd_last_direct_outputs(void);
const char *dd_last_error(void);
int dd_abi_version(void);
int dd_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* DINDEL_HMM_H */
